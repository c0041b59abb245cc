"""Client helpers.

`generate_text` keeps the notebook helper's signature and return contract
(`/root/reference/notebook.ipynb:111-120`): the parsed JSON dict on HTTP 200,
otherwise the string "Error: {code} - {text}"; network failures return
"Request failed: {exc}".  The optional sampling fields of /generate
(temperature, top_k, top_p, min_p, presence_penalty, frequency_penalty, logprobs,
logit_bias, banned_token_ids, min_new_tokens, repetition_penalty,
no_repeat_ngram_size, allowed_token_ids, bad_words, bad_words_ids, stop,
stop_token_ids, include_stop_in_output, guided_regex, guided_choice, n, greedy, seed,
stop_at_eos) are sent
when given; with logprobs the returned dict
has a "logprobs" object beside "generated", with stop or stop_token_ids a
"finish_reason" and, after a stop, a "stop_reason"; with n > 1 "generated" is
sample 0 and "choices" holds one such object per sample.
"""
from __future__ import annotations

import os
from typing import Union

COORDINATOR_URL = os.environ.get("COORDINATOR_URL", "http://127.0.0.1:5000/generate")


def generate_text(prompt: str, max_new_tokens: int = 20, url: str = None,
                  timeout: float = 300.0, top_p: float = None, min_p: float = None,
                  presence_penalty: float = None, frequency_penalty: float = None,
                  logprobs: int = None, logit_bias: dict = None, banned_token_ids: list = None,
                  min_new_tokens: int = None, repetition_penalty: float = None,
                  no_repeat_ngram_size: int = None, allowed_token_ids: list = None, bad_words: list = None,
                  bad_words_ids: list = None, stop=None, stop_token_ids: list = None,
                  include_stop_in_output: bool = None, guided_regex: str = None,
                  guided_choice: list = None, n: int = None, **sampling) -> Union[dict, str]:
    import requests

    payload = {"prompt": prompt, "max_new_tokens": max_new_tokens}
    sampling.update(top_p=top_p, min_p=min_p, presence_penalty=presence_penalty,
                    frequency_penalty=frequency_penalty, logprobs=logprobs, logit_bias=logit_bias,
                    banned_token_ids=banned_token_ids, min_new_tokens=min_new_tokens,
                    repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                    allowed_token_ids=allowed_token_ids, bad_words=bad_words, bad_words_ids=bad_words_ids,
                    stop=stop, stop_token_ids=stop_token_ids, include_stop_in_output=include_stop_in_output,
                    guided_regex=guided_regex, guided_choice=guided_choice, n=n)
    payload.update({k: v for k, v in sampling.items() if v is not None})
    try:
        r = requests.post(url or COORDINATOR_URL, json=payload, timeout=timeout)
        if r.status_code == 200:
            return r.json()
        return f"Error: {r.status_code} - {r.text}"
    except requests.exceptions.RequestException as e:
        return f"Request failed: {e}"
