"""Exact-arithmetic probes (tests/norm_probes.py) on every instantiation that
lsd_norm (csrc/kernels/norm.hip) can launch, on an MI355X: the block-per-row
kernel (MAXV 2 / 4 / 8, 0 .. 8 unrolled slabs and the runtime loop, fp32 and
bf16 slabs, fold-only), the wave-per-row kernel (MAXC 4 / 8 / 16, 1 .. 8 slabs at
H <= 1024) and the fold-first pair.  Every launch asserts, through
C.norm_last_launch(), that the kernel it meant to exercise is the one that ran.

x is always the first T rows of a larger buffer whose other rows hold SENTINEL,
and the whole buffer is compared bit for bit after the launch.  Slabs are
tested together with the norm: x0 = probe row - (slabs + pending bias), all
integers below 2^24, so the fold must give back the probe's row exactly (any
wrong split, row or column leaves a coded integer behind) and the output is the
probe's.  Widths are both sides of every MAXV / MAXC step, of thread 255 -> the
second column group and of the lane wrap; T = 5 (block) and 1, 4, 5, 9 (wave:
partial last blocks of 4 rows).
"""
import functools

import pytest
import torch

from . import norm_probes as npb
from .test_kernels_gpu import _norm_defaults

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
EPS = (1e-5, 1e-3)
BLOCK_H = (4, 8, 12, 1020, 1024, 1028, 2048, 2052, 4096, 4100, 8192)
WAVE_H = (4, 252, 256, 260, 1024, 1028, 1036, 2048, 2052, 4096)
WAVE_SLAB_H = (4, 252, 256, 260, 1024)
FOLD_FIRST = ((252, (9, 12)), (1024, (9, 12)), (1600, (1, 2, 3, 4, 5, 6, 7, 8, 9, 12)),
              (2052, (1, 2, 3, 4, 5, 6, 7, 8, 9)))
WAVE_T = (1, 4, 5, 9)
SLABS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12)
TAGS = set()   # every launch tag observed
RAN = []       # one entry per variant test that ran (test_every_norm_instantiation_was_reached)
WORST = {}     # figure -> largest value seen (printed by the last test)


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


@pytest.fixture(autouse=True)
def _thresholds(C):
    """Block kernel unless a test turns the wave kernel on; defaults afterwards."""
    C.norm_set_wave_min(0)
    C.norm_set_wave_narrow_min(0)
    try:
        yield
    finally:
        _norm_defaults(C)


def worst(name, v):
    WORST[name] = max(WORST.get(name, 0.0), v)
    return v


def kind_of(rms):
    return "rms" if rms else "ln"


def block_tag(H, kind, S=0, sdt=None):
    mv = 2 if H <= 2048 else 4 if H <= 4096 else 8
    s = f"s{S}" if S <= 8 else "loop"
    return f"block<{mv},{kind},{s}" + ("" if S == 0 else ",bf16" if sdt == BF else ",f32") + ">"


def wave_tag(H, kind, S=0, sdt=None):
    mc = 4 if H <= 1024 else 8 if H <= 2048 else 16
    return f"wave<{mc},{kind}" + ("" if S == 0 else f",s{S}," + ("bf16" if sdt == BF else "f32")) + ">"


def every_tag():
    """What lsd_norm's branches can record for H <= 8192 and >= 1 slab when
    slabs are given (restated from the dispatch, not read from it)."""
    tags = set()
    counts = [f"s{i}" for i in range(1, 9)] + ["loop"]
    for mv in (2, 4, 8):
        for kind in ("ln", "rms", "fold"):
            tags.add(f"block<{mv},{kind},s0>")
            tags |= {f"block<{mv},{kind},{s},{dt}>" for s in counts for dt in ("f32", "bf16")}
    for kind in ("ln", "rms"):
        tags |= {f"wave<{mc},{kind}>" for mc in (4, 8, 16)}
        tags |= {f"wave<4,{kind},s{i},{dt}>" for i in range(1, 9) for dt in ("f32", "bf16")}
        for dt in ("f32", "bf16"):  # fold first: other counts at H <= 1024, any count above
            tags.add(f"block<2,fold,loop,{dt}>+wave<4,{kind}>")
            tags |= {f"block<2,fold,{s},{dt}>+wave<8,{kind}>" for s in counts}
            tags |= {f"block<4,fold,{s},{dt}>+wave<16,{kind}>" for s in counts}
    return tags


@functools.lru_cache(maxsize=None)
def sign(T, H, rms, kind="wide"):
    return npb.sign_case(T, H, rms, kind)


@functools.lru_cache(maxsize=None)
def offset(T, H, kind):
    return npb.offset_case(T, H, kind)


@functools.lru_cache(maxsize=None)
def null(T, H, eps):
    return npb.null_case(T, H, eps)


@functools.lru_cache(maxsize=None)
def folded(T, H, S, sdt, bias):
    """(delta fp32 [T, H] on the CPU, slab, pending bias on the GPU): what the
    slabs and the bias add to every row."""
    f = npb.fold_case(T, H, S, sdt, bias)
    return f.x_exp - f.x, f.slab.to(DEV), None if f.pbias is None else f.pbias.to(DEV)


def guarded_rows(x, extra=3):
    """(buffer, its first T rows): the rows after them hold SENTINEL."""
    buf = torch.full((x.shape[0] + extra, x.shape[1]), npb.SENTINEL, dtype=F32, device=DEV)
    buf[:x.shape[0]] = x.to(DEV)
    return buf, buf[:x.shape[0]]


def run(C, c, x_rows, rms, tag, *, eps=1e-5, S=0, sdt=F32, bias=True, rows=None, want=True):
    """One launch on the probe rows `x_rows` (CPU fp32, integers when S > 0):
    asserts the tag, the folded residual and every guard row; returns (out,
    the residual rows)."""
    T, H = x_rows.shape
    slab = pb = None
    x0 = x_rows
    if S:
        delta, slab, pb = folded(T, H, S, sdt, bias)
        x0 = x_rows - delta
        assert float(x0.abs().max()) < 2.0 ** 24 and torch.equal(x0 + delta, x_rows)
    buf, xv = guarded_rows(x0)
    out = C.norm(xv, slab, pb, c.w.to(DEV) if want else None, c.b.to(DEV) if want and not rms else None, eps, rms,
                 rows, want)
    got = C.norm_last_launch()
    TAGS.add(got)
    assert got == tag, f"meant to run {tag}, ran {got}"
    ebuf, _ = guarded_rows(x_rows)
    assert npb.bits_equal(buf, ebuf), f"{tag}: residual or the rows after it (S {S}, bias {bias})"
    assert (out is None) == (not want)
    return out, xv


def check_probes(C, T, H, rms, tag):
    """The slab-free probes on whichever kernel the thresholds select."""
    kind = kind_of(rms)
    c = sign(T, H, rms)
    out, _ = run(C, c, c.x, rms, tag)
    assert npb.bits_equal(out, c.out_exp.to(DEV)), "sign probe: gamma placement"
    for eps in EPS:
        e = npb.eps_case(T, H, rms, eps)
        out, _ = run(C, e, e.x, rms, tag, eps=eps)
        r = worst(f"eps {tag.split('<')[0]} {kind}", npb.rel_err(out, e.exp))
        assert r <= npb.REL_TOL, f"eps probe (eps {eps:g}): {r:.3e} relative, tolerance {npb.REL_TOL:.3e}"
    if rms:
        return
    c = sign(T, H, False, "beta")
    out, _ = run(C, c, c.x, False, tag)
    assert npb.bits_equal(out, c.out_exp.to(DEV)), "sign probe: beta placement"
    for k in ("wide", "beta"):
        c = offset(T, H, k)
        out, _ = run(C, c, c.x, False, tag)
        assert npb.bits_equal(out, c.out_exp.to(DEV)), f"offset probe ({k})"
    for eps in EPS:
        c = null(T, H, eps)
        out, _ = run(C, c, c.x, False, tag, eps=eps)
        r = worst(f"null {tag.split('<')[0]} ln", npb.null_ratio(out, c))
        print(f"null probe {tag} T {T} H {H} eps {eps:g}: err / bound = {r:.4f}")
        assert r <= 1.0, f"null probe (eps {eps:g}): err / bound = {r:.3f}, bound {c.bound:.3e}"


def check_energy(C, H, kind, tag):
    rms = kind == "rms"
    c = npb.energy_case(H, rms, kind == "ln_unbalanced", device=DEV)
    assert c.x.shape == (H // 4, H)
    out, _ = run(C, c, c.x, rms, tag)
    r = worst(f"energy {tag.split('<')[0]} {kind}", npb.rel_err(out, c.exp))
    assert r <= npb.REL_TOL, f"energy probe: {r:.3e} relative, tolerance {npb.REL_TOL:.3e}"


def check_isolation(C, T, H, rms, S, sdt, tag):
    """The probe's rows interleaved with NaN rows (slabs likewise): bit-equal
    to the launch without them."""
    c = sign(T, H, rms)
    w, b = c.w.to(DEV), None if rms else c.b.to(DEV)
    delta, slab, pb = folded(T, H, S, sdt, True)
    x1 = (c.x - delta).to(DEV)
    x2 = npb.interleave_nan(x1)
    out1 = C.norm(x1, slab, pb, w, b, 1e-5, rms, None, True)
    assert C.norm_last_launch() == tag
    out2 = C.norm(x2, npb.interleave_nan(slab, 1), pb, w, b, 1e-5, rms, None, True)
    assert C.norm_last_launch() == tag
    assert npb.bits_equal(out1, c.out_exp.to(DEV)) and npb.bits_equal(x1, c.x.to(DEV))
    assert npb.bits_equal(out2[0::2], out1) and npb.bits_equal(x2[0::2], x1), "a row's result depends on its neighbours"
    assert bool(torch.isnan(x2[1::2]).all())


# ---------------------------------------------------------------------------
# block-per-row kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("H", BLOCK_H)
def test_block_fold_and_norm(C, H, rms):
    """Every unrolled slab count and the runtime loop, fp32 and bf16 slabs,
    with and without the pending bias, norm requested and fold-only."""
    T, kind = 5, kind_of(rms)
    c = sign(T, H, rms)
    exp = c.out_exp.to(DEV)
    for S in SLABS:
        for sdt in ((F32, BF) if S else (F32,)):
            for bias in ((True, False) if S else (False,)):
                out, _ = run(C, c, c.x, rms, block_tag(H, kind, S, sdt), S=S, sdt=sdt, bias=bias)
                assert npb.bits_equal(out, exp), (S, sdt, bias)
                run(C, c, c.x, rms, block_tag(H, "fold", S, sdt), S=S, sdt=sdt, bias=bias, want=False)
    RAN.append(("block_fold", H, rms))


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("H", BLOCK_H)
def test_block_probes(C, H, rms):
    """eps, offset, null and beta placement; the row gather; isolation."""
    T, kind = 5, kind_of(rms)
    tag = block_tag(H, kind)
    check_probes(C, T, H, rms, tag)
    c = sign(T, H, rms)
    rows = torch.tensor([3, 0, 4, 3, 1], dtype=torch.int32, device=DEV)
    plain, _ = run(C, c, c.x, rms, tag)
    out, _ = run(C, c, c.x, rms, tag, rows=rows)  # run() asserts x and its guards are bit-unchanged
    assert npb.bits_equal(out, c.out_exp.to(DEV)[rows.long()]) and npb.bits_equal(out, plain[rows.long()])
    out, _ = run(C, c, c.x, rms, tag, rows=rows[:2])
    assert out.shape == (2, H) and npb.bits_equal(out, plain[rows[:2].long()])
    check_isolation(C, T, H, rms, 2, F32, block_tag(H, kind, 2, F32))
    check_isolation(C, T, H, rms, 9, BF, block_tag(H, kind, 9, BF))
    RAN.append(("block_probes", H, rms))


@pytest.mark.parametrize("kind", ["rms", "ln", "ln_unbalanced"])
@pytest.mark.parametrize("H", BLOCK_H)
def test_block_energy(C, H, kind):
    """One row per 16-byte chunk: every chunk counted once, the divisor is H."""
    check_energy(C, H, kind, block_tag(H, "rms" if kind == "rms" else "ln"))
    RAN.append(("block_energy", H, kind))


# ---------------------------------------------------------------------------
# wave-per-row kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("H", WAVE_H + (4100,))
def test_wave_probes(C, H, rms):
    """Every MAXC, 1 .. 9 rows; 4100 columns stay on the block kernel."""
    C.norm_set_wave_min(1)
    tag = wave_tag(H, kind_of(rms)) if H <= 4096 else block_tag(H, kind_of(rms))
    for T in WAVE_T:
        check_probes(C, T, H, rms, tag)
    RAN.append(("wave_probes", H, rms))


@pytest.mark.parametrize("kind", ["rms", "ln", "ln_unbalanced"])
@pytest.mark.parametrize("H", WAVE_H)
def test_wave_energy(C, H, kind):
    C.norm_set_wave_min(1)
    check_energy(C, H, kind, wave_tag(H, "rms" if kind == "rms" else "ln"))
    RAN.append(("wave_energy", H, kind))


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("H", WAVE_SLAB_H)
def test_wave_slabs(C, H, rms):
    """1 .. 8 slabs folded in the wave kernel (narrow threshold).  The folded
    residual is the one right bit pattern, which test_block_fold_and_norm
    holds the block kernel to as well: the two are bit-equal."""
    C.norm_set_wave_narrow_min(1)
    kind = kind_of(rms)
    for T in WAVE_T:
        c = sign(T, H, rms)
        exp = c.out_exp.to(DEV)
        for S in range(1, 9):
            for sdt in (F32, BF):
                for bias in (True, False):
                    out, _ = run(C, c, c.x, rms, wave_tag(H, kind, S, sdt), S=S, sdt=sdt, bias=bias)
                    assert npb.bits_equal(out, exp), (T, S, sdt, bias)
        if not rms:
            for eps in EPS:
                n = null(T, H, eps)
                for S, sdt in ((1, BF), (3, F32), (8, BF)):
                    out, _ = run(C, n, n.x, False, wave_tag(H, "ln", S, sdt), eps=eps, S=S, sdt=sdt)
                    r = worst("null wave+slabs ln", npb.null_ratio(out, n))
                    assert r <= 1.0, f"null probe with {S} slabs (eps {eps:g}): err / bound = {r:.3f}"
            c = offset(T, H, "wide")
            out, _ = run(C, c, c.x, False, wave_tag(H, "ln", 5, F32), S=5, sdt=F32)
            assert npb.bits_equal(out, c.out_exp.to(DEV))
    check_isolation(C, 5, H, rms, 2, F32, wave_tag(H, kind, 2, F32))
    check_isolation(C, 5, H, rms, 7, BF, wave_tag(H, kind, 7, BF))
    RAN.append(("wave_slabs", H, rms))


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("H,counts", FOLD_FIRST)
def test_wave_fold_first(C, H, counts, rms):
    """Other slab counts at H <= 1024 and any count above: the block kernel's
    fold-only pass, then the slab-free wave kernel -- both launches recorded."""
    C.norm_set_wave_min(1)
    T, kind = 5, kind_of(rms)
    c = sign(T, H, rms)
    for S in counts:
        for sdt in (F32, BF):
            tag = block_tag(H, "fold", S, sdt) + "+" + wave_tag(H, kind)
            out, _ = run(C, c, c.x, rms, tag, S=S, sdt=sdt, bias=S % 2 == 1)
            assert npb.bits_equal(out, c.out_exp.to(DEV)), (S, sdt)
    S = counts[-1]
    check_isolation(C, T, H, rms, S, BF, block_tag(H, "fold", S, BF) + "+" + wave_tag(H, kind))
    if not rms:
        n = null(T, H, 1e-5)
        out, _ = run(C, n, n.x, False, block_tag(H, "fold", S, F32) + "+" + wave_tag(H, "ln"), S=S, sdt=F32)
        assert worst("null wave+slabs ln", npb.null_ratio(out, n)) <= 1.0
    RAN.append(("fold_first", H, rms))


def test_every_norm_instantiation_was_reached():
    """Runs last: the tests above recorded every tag that lsd_norm's dispatch
    can produce (a deselected run proves nothing here)."""
    print("norm tags:", len(TAGS), sorted(TAGS))
    print("worst figures:", {k: float(f"{v:.4g}") for k, v in sorted(WORST.items())})
    n = 2 * 2 * len(BLOCK_H) + 3 * len(BLOCK_H) + 2 * (len(WAVE_H) + 1) + 3 * len(WAVE_H) + 2 * len(WAVE_SLAB_H) \
        + 2 * len(FOLD_FIRST)
    if len(RAN) < n:
        return
    want = every_tag()
    assert TAGS == want, (sorted(want - TAGS), sorted(TAGS - want))
