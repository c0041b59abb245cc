"""plan_gemm() (csrc/kernels/gemm_plan.h), the one place a GEMM launch is
decided, against tests/gemm_plan_model.py: the launch rules as the launchers,
the sizing queries and run_gemm held them before the header, transcribed to
Python.  A stand-alone driver (csrc/kernels/tests/gemm_plan_driver.cpp) built
with AddressSanitizer + UBSan prints the plans.  A wrong grid, counter count
or workspace size would be an out-of-bounds write on the GPU; here it is a
failed comparison.  CPU only."""
import os
import re
import shutil
import subprocess

import pytest

from . import gemm_plan_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MS = (1, 16, 17, 64, 65, 96, 97, 128, 129, 192, 256, 257, 512, 1024, 1025, 4096)
NS = (64, 96, 128, 192, 768, 1600, 4800, 6400, 50304)
KS = (64, 96, 128, 768, 1600, 4096, 8192)
SS = (1, 2, 3, 8)
# The combined-knob sets below keep every M (the row boundaries), every split
# count, epilogue and kind.  The rules read N through N % 32 / 64 / 128 and the
# tile counts, K only through K % 64: one N of every residue class at a small,
# a middle and the vocabulary width, and both classes of K.
NS_THIN = (64, 96, 192, 768, 6400, 50304)
KS_THIN = (64, 96, 4096)

DEFAULT = {}
# what HipBackend.__init__ applies from Routing() (ops/routing.py defaults)
PRODUCTION = dict(sk_rows=64, big_min_blocks=160, nw2_rows=1 << 30, tiled3_max_blocks=512, ring_slots=3, ring_tn=0,
                  ring_fill=128, ring_m96=0, d256_slots=3, ring8=2, ring8_flags=0)
# every value tests/test_gemm_exact_gpu.py and tests/test_kernels_gpu.py set
MOVES = dict(big_min_blocks=(1, 160), big_group=(0, 4), big_kind=(0, 1, 4), tiled3_max_blocks=(0, 512, 1 << 30),
             ring_slots=(3, 4), ring_tn=(0, 32, 64, 128), ring_fill=(128,), ring_m96=(0, 1 << 30), ring8=(0, 1, 2),
             ring8_flags=(0, 1, 2, 4), ring8_pack=(0, 1, 2, 3), d256_slots=(2, 3, 4), nw2_rows=(0, 1 << 30),
             sk_rows=(64, 128))


def knob_sets():
    """(name, knobs, Ns, Ks): the two bases over the whole sweep, then each
    knob moved alone from either base to every value the GPU tests set."""
    sets = [("default", DEFAULT, NS, KS), ("production", PRODUCTION, NS, KS)]
    for base_name, base in (("default", DEFAULT), ("production", PRODUCTION)):
        for knob, values in MOVES.items():
            for v in values:
                if dict(model.DEFAULTS, **base)[knob] != v:
                    sets.append((f"{base_name}+{knob}={v}", dict(base, **{knob: v}), NS, KS))
    # the knobs as the GPU tests combine them (ring_knobs, ring8_knobs): some
    # instances need two knobs moved, e.g. the 4-slot ring under a ring cap
    uncapped = dict(tiled3_max_blocks=1 << 30)
    for slots, tn, m96 in ((3, 128, 0), (4, 128, 0), (3, 64, 0), (3, 32, 0), (3, 0, 0), (3, 64, 1 << 30)):
        sets.append((f"ring {slots} {tn} {m96}", dict(uncapped, ring_slots=slots, ring_tn=tn, ring_m96=m96),
                     NS_THIN, KS_THIN))
    for var, flags, pack in ((1, 0, 0), (2, 0, 0), (2, 1, 0), (2, 2, 0), (2, 4, 0), (2, 0, 1), (2, 0, 2), (2, 0, 3)):
        sets.append((f"ring8 {var} {flags} {pack}", dict(uncapped, ring_tn=64, ring8=var, ring8_flags=flags,
                                                         ring8_pack=pack), NS_THIN, KS_THIN))
    return sets


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("gemm_plan") / "driver"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "csrc", "kernels", "tests", "gemm_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in r.stderr:
        pytest.skip(f"sanitizer runtime not available: {r.stderr[-200:]}")
    assert r.returncode == 0, r.stderr

    def run(script):
        env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
        r = subprocess.run([str(exe)], input=script, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout.splitlines()

    return run


def knob_lines(kn):
    return "reset\n" + "".join(f"knob {k} {v}\n" for k, v in kn.items())


def line(p):
    valid, tag, grid, block, tiles, floats = p
    return f"1 {tag} {grid[0]} {grid[1]} {grid[2]} {block} {tiles} {floats}" if valid else "0"


def test_plans_equal_the_model(driver):
    sets = knob_sets()
    script = []
    for _, kn, ns, ks in sets:
        script.append(knob_lines(kn) + "".join(f"{n} {' '.join(map(str, v))}\n"
                                               for n, v in (("M", MS), ("N", ns), ("K", ks), ("S", SS))) + "sweep\n")
    got = driver("".join(script))
    at, seen = 0, set()
    for name, kn, ns, ks in sets:
        k = model.knobs(**kn)
        cases = [(M, N, K, S, epi, kind) for M in MS for N in ns for K in ks for S in SS for epi in range(7)
                 for kind in range(4)]
        want = [line(model.plan(k, *c)) for c in cases]
        have = got[at:at + len(want)]
        at += len(want)
        if have != want:
            i = next(i for i, (a, b) in enumerate(zip(have, want)) if a != b)
            pytest.fail(f"{name}: (M, N, K, splits, epi, kind) = {cases[i]}: plan {have[i]!r}, model {want[i]!r}")
        seen.update(have)
    assert at == len(got)
    # every family and every in-kernel combine was in the sweep
    tags = {ln.split()[1] for ln in seen if ln != "0"}
    assert "0" in seen and {"tiled", "big", "p8<0>", "p8<4>", "ring<3,32>", "ring<3,64>", "ring<3,64,m96>",
                            "ring<3,128>", "ring<4,128>", "ring8<1,3>", "ring8<2,3>", "ring8<2,3,nt>", "ring8<2,3,bl>",
                            "ring8<2,3,pk1>", "ring8<2,3,pk2>", "ring8<2,3,pk3>", "d256<64,2>", "d256<64,3>",
                            "d256<64,4>", "d256<128,2>", "d256<128,3>"} <= tags
    assert {f"sk<{mt},{nw}>" for mt in (1, 2, 3, 4, 6, 8) for nw in (1, 2)} <= tags
    # outright, whatever the model says: a launchable grid, an instantiated MT,
    # and the workspace floats the chosen kernel indexes by its tile shape
    combined = set()
    for ln in seen - {"0"}:
        _, tag, gx, gy, gz, block, tiles, floats = ln.split()
        assert int(gx) > 0 and int(gy) > 0 and int(gz) > 0 and int(block) in (256, 512), ln
        assert (int(tiles) > 0) == (int(floats) > 0), ln
        m = re.fullmatch(r"sk<(\d),(\d)>", tag)
        if m:
            assert int(m.group(1)) in (1, 2, 3, 4, 6, 8) and int(m.group(2)) in (1, 2), ln
        if int(tiles):
            combined.add(tag.split("<")[0])
            if m:
                assert int(floats) == int(m.group(1)) * 16 * 64 * int(m.group(2)), ln
                assert int(tiles) == int(gx) * int(gz), ln
            elif tag.startswith("d256<"):
                assert int(floats) == 256 * int(tag[5:].split(",")[0]), ln
            else:
                assert tag.startswith("ring8<2,3") and int(floats) == 128 * 64, ln
    assert combined == {"sk", "d256", "ring8"}


def test_refusals(driver):
    """Invalid exactly where the launchers returned hipErrorInvalidValue for
    shape or knob reasons -- and for shapes run_gemm never let through."""
    ring8 = dict(tiled3_max_blocks=1 << 30, ring_tn=64)
    cases = [
        ({}, "128 128 128 1 7 0"), ({}, "128 128 128 1 -1 1"),                  # unknown epilogue
        # (a split-K MT outside {1, 2, 3, 4, 6, 8} needs M < 1: row blocks hold at most 128 rows)
        ({}, "1025 128 128 1 0 2"), ({}, "256 128 96 1 0 3"),                   # d256_bn == 0
        (dict(ring8, ring8=1), "128 128 128 2 0 1"), (ring8, "128 128 128 2 4 1"),  # combine without ring8 == 2
        ({}, "0 128 128 1 0 0"), ({}, "128 0 128 1 0 1"), ({}, "128 128 128 0 0 2"),
    ]
    valid = [
        (dict(ring8, ring8=2), "128 128 128 2 0 1"),   # the same launch on the all-compute ring
        (dict(ring8, ring8=1), "128 128 128 2 5 1"),   # slabs: no combine
        ({}, "1024 128 128 1 0 2"), ({}, "256 128 128 1 0 0"),
        ({}, "128 128 128 2 0 1"),                     # no combine kernel, not refused here: run_gemm raises
    ]
    got = driver("".join(knob_lines(kn) + f"plan {c}\n" for kn, c in cases + valid))
    assert got[:len(cases)] == ["0"] * len(cases)
    assert all(ln.startswith("1 ") for ln in got[len(cases):]) and len(got) == len(cases) + len(valid)
    for (kn, c), ln in zip(cases + valid, got):
        assert ln == line(model.plan(model.knobs(**kn), *map(int, c.split()))), c
    assert got[len(cases)].split()[1] == "ring8<2,3>" and got[-1] == "1 tiled 2 1 1 256 0 0"


def test_setters_clamp(driver):
    """GemmTuning's defaults, and the lsd_gemm_set_* rules: out-of-range
    values land where they did."""
    clamps = [("ring_tn", 48, 128), ("ring_tn", 32, 32), ("sk_rows", 1, 16), ("sk_rows", 1000, 128),
              ("d256_slots", 1, 2), ("d256_slots", 9, 4), ("ring8_flags", 9, 1), ("ring8_pack", 6, 2),
              ("big_kind", 2, 0), ("big_kind", 1, 1), ("big_group", -3, 0), ("ring_slots", 5, 3), ("ring_slots", 4, 4),
              ("ring8", 3, 0), ("ring8", 2, 2), ("big_min_blocks", -5, -5), ("nw2_rows", 0, 0), ("rb_fill", 7, 7)]
    got = driver("reset\nshow\n" + "".join(f"reset\nknob {k} {v}\nshow\n" for k, v, _ in clamps))
    assert got[0].split() == [str(v) for v in model.DEFAULTS.values()]
    assert model.DEFAULTS == dict(big_min_blocks=160, big_group=4, big_kind=4, tiled3_max_blocks=0, ring_slots=3,
                                  ring_tn=128, ring_fill=128, ring_m96=0, ring8=0, ring8_flags=0, ring8_pack=0,
                                  d256_slots=3, sk_rows=64, rb_fill=192, nw2_rows=1 << 30)
    for (knob, v, lands), ln in zip(clamps, got[1:]):
        assert ln.split() == [str(x) for x in dict(model.DEFAULTS, **{knob: lands}).values()], (knob, v)
        assert model.knobs(**{knob: v})[knob] == lands, (knob, v)
