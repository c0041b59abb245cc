"""Exact-arithmetic probes (tests/gemm_probes.py) on every GEMM / GEMV kernel
variant and epilogue of csrc/kernels/gemm.hip and gemv.hip, on an MI355X.

Integer inputs whose products and sums are exact give one right bit pattern
per output whatever the kernel, tile shape, split count or ring depth; every
launch also asserts, through C.gemm_last_launch(), that the kernel variant it
meant to exercise is the one that ran.  Operands are strided views of one
larger operand per family (row stride > K); the residual and the KV caches
sit between sentinel guards that are compared bit for bit after the launch.

Shapes are the smallest that cross each edge of the tile constants in
gemm.hip: 16-row MFMA tiles and the 64 / 128-row blocks of gemm_sk, its 128 /
256 / 512-k rounds, the 96 / 128 / 256-row and 32 / 64 / 128 / 256-column tiles
of the tiled families, k-steps fewer than, equal to and more than each ring.
"""
import math
from types import SimpleNamespace

import pytest
import torch

from llm_sharding_demo_amd.ops.hip import interleave_gate_up

from . import gemm_probes as gp

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
TAGS = set()       # every launch tag observed
ACT_WORST = {}     # kernel family -> largest activation error / bound
RAN = []           # one entry per variant test that ran (test_every_launch_branch_was_reached)


@pytest.fixture(scope="module")
def C():
    from llm_sharding_demo_amd.ops.hip import _load

    return _load()


@pytest.fixture(scope="module")
def CNT():
    return torch.zeros(1 << 16, dtype=torch.int32, device=DEV)


def _defaults(C):
    """The launch knobs' values in gemm.hip / gemv.hip (what
    tests/test_kernels_gpu.py's fixtures restore as well)."""
    C.gemm_set_big_min(160)
    C.gemm_set_big_group(4)
    C.gemm_set_big_kind(4)
    C.gemm_set_tiled3_max(0)
    C.gemm_set_ring_slots(3)
    C.gemm_set_ring_tn(128)
    C.gemm_set_ring_fill(128)
    C.gemm_set_ring_m96(0)
    C.gemm_set_ring8(0)
    C.gemm_set_ring8_flags(0)
    C.gemm_set_ring8_pack(0)
    C.gemm_set_d256_slots(3)
    C.gemm_set_nw2_rows(1 << 30)
    C.gemm_set_sk_rows(64)
    C.gemv_set_nt(0)


@pytest.fixture(autouse=True)
def _knobs(C):
    prev = C.gemm_slab_bf16()
    _defaults(C)
    yield
    _defaults(C)
    C.gemm_set_slab_bf16(int(prev))


def dev(t, dtype=BF):
    return t.to(dtype).to(DEV)


class Data:
    """One integer probe per kernel family, built once: operands at the
    largest (M, N, K) of the family, cut to each case as strided views; exact
    products per K, computed once on the CPU in fp64 and kept on the GPU."""

    def __init__(self, Mmax, Nmax, Kmax, seed):
        self.ai, self.wi, self.bi, self.xi = gp.integer_operands(Mmax, Nmax, Kmax, seed)
        self.wwi = gp.wide_weights(self.wi, seed)
        # every partial sum over whole 32-k blocks, of any prefix K: a bf16 number even with the bias
        assert gp.max_partial_range(self.ai, self.wi) + 8 <= gp.BF16_INT
        self.a, self.w, self.ww, self.bias = dev(self.ai), dev(self.wi), dev(self.wwi), dev(self.bi)
        self.x = dev(self.xi, torch.float32)
        self._y, self._silu, self._qkvw, self._qkv = {}, {}, {}, {}

    def y(self, K, wide=False):
        """fp64 [Mmax, Nmax] on the GPU: the exact a[:, :K] w[:, :K]^T."""
        if (K, wide) not in self._y:
            y = gp.exact_product(self.ai[:, :K], (self.wwi if wide else self.wi)[:, :K])
            if not wide:
                gp.assert_bf16_exact(y, self.bi)
            self._y[(K, wide)] = y.double().to(DEV)
        return self._y[(K, wide)]

    def silu(self, Ns, K, which):
        """(a, interleaved w) at full size and the exact (gate, up) [Mmax, Ns / 2] of the probe at K."""
        if (Ns, which) not in self._silu:
            a, w, _, _ = gp.silu_operands(self.ai, self.wi[:Ns], which)
            self._silu[(Ns, which)] = (a, w, dev(a), interleave_gate_up(dev(w), Ns // 2).contiguous(), {})
        a, w, ad, wd, ys = self._silu[(Ns, which)]
        if K not in ys:
            y = gp.exact_product(a[:, :K], w[:, :K])
            gp.assert_bf16_exact(y[:, Ns // 2:])
            ys[K] = (y[:, :Ns // 2].double().to(DEV), y[:, Ns // 2:].double().to(DEV))
        return ad, wd, ys[K]

    def qkv_weights(self, N, rope):
        """(w, bias) cut to N columns, in the RoPE epilogue's row order when rope."""
        if (N, rope) not in self._qkvw:
            perm = (gp.qkv_weight_order(N) if rope else torch.arange(N)).to(DEV)
            self._qkvw[(N, rope)] = (self.w[:N][perm].contiguous(), self.bias[:N][perm].contiguous())
        return self._qkvw[(N, rope)]

    def qkv(self, M, N, K, rope):
        """Token map, RoPE table and the expected q / cache buffers on the GPU."""
        key = (M, N, K, rope)
        if key not in self._qkv:
            if len(self._qkv) > 64:
                self._qkv.clear()
            tslot, tpos, S = gp.token_map(M)
            hd = gp.qkv_dims(N)[2]
            table = gp.rope_table_exact(S, hd) if rope else None
            yb = (self.y(K)[:M, :N].cpu() + self.bi[:N][None, :]).long()
            q, ek, ev = gp.qkv_expected(yb, N, tslot, tpos, 3, S, table)
            self._qkv[key] = (tslot.to(DEV), tpos.to(DEV), S, None if table is None else table.to(DEV),
                              q.to(DEV), ek.to(DEV), ev.to(DEV))
        return self._qkv[key]


_DATA = {}


def data(name):
    shapes = {"sk": (256, 256, 1600, 0), "tiled": (257, 352, 640, 1), "ring8": (257, 352, 1600, 2),
              "big": (513, 320, 640, 3), "d256": (1024, 384, 1600, 4), "routed": (300, 4160, 1280, 5),
              "blaslt": (512, 320, 640, 6)}
    if name not in _DATA:
        _DATA[name] = Data(*shapes[name])
    return _DATA[name]


def tagged(C, tag):
    got = C.gemm_last_launch()
    TAGS.add(got)
    assert got == tag, f"meant to run {tag}, ran {got}"


def act_ok(family, out, name, pre, scale=None):
    r = gp.act_ratio(out, name, pre, scale)
    ACT_WORST[family] = max(ACT_WORST.get(family, 0.0), r)
    assert r <= 1.0, f"{name}: error / bound = {r}"


def fold(C, x, slab, bias):
    C.norm(x, slab, bias, None, None, 0.0, True, None, False)


def run_epilogues(C, CNT, D, family, M, N, K, kind, splits, tag, *, combine=True, silu_n=None, silu_tag=None):
    """Every epilogue of one (variant, shape, splits) on the integer probe.
    combine: the variant sums its splits in the kernel (any epilogue at
    splits > 1); else splits > 1 exists only as residual slabs."""
    a, w, ww, bias = D.a[:M, :K], D.w[:N, :K], D.ww[:N, :K], D.bias[:N]
    y, yw = D.y(K)[:M, :N], D.y(K, True)[:M, :N]
    yb = y + bias.double()[None, :]
    xe = D.x[:M, :N].double()
    direct = splits == 1 or combine
    if direct:
        out = C.linear(a, w, bias, 0, kind, splits, CNT)
        tagged(C, tag)
        assert gp.same_values(out, yb), "bf16 + bias"
        out = C.linear(a, w, bias, 1, kind, splits, CNT)
        tagged(C, tag)
        act_ok(family, out, "gelu", yb)
        Ns = (N // 32 * 32) if silu_n is None else silu_n
        for which in ("up", "gate"):
            ad, wd, (gate, up) = D.silu(Ns, K, which)
            out = C.linear(ad[:M, :K], wd[:, :K], None, 2, kind, splits, CNT)
            tagged(C, silu_tag or tag)
            if which == "up":
                assert gp.same_values(out, 32 * up[:M]), "silu(32) * up"
            else:
                act_ok(family, out, "silu", gate[:M])
        out = C.linear_f32(a, ww, kind, splits, CNT)
        tagged(C, tag)
        assert out.dtype == torch.float32 and gp.same_values(out, yw), "fp32"
        if kind:  # the tiled kinds also write the 8-column segment maxima
            seg = torch.full((M, N // 8), float("nan"), device=DEV)
            out = C.linear_f32(a, ww, kind, splits, CNT, seg)
            tagged(C, tag)
            assert gp.same_values(out, yw) and gp.same_values(seg, gp.segmax_expected(yw)), "fp32 + segmax"
        for rope in (False, True):
            tslot, tpos, S, table, q_exp, ek, ev = D.qkv(M, N, K, rope)
            qs, kvs, hd, nh, nkv = gp.qkv_dims(N)
            wq, bq = D.qkv_weights(N, rope)
            kb = torch.full((5, nkv, S, hd), gp.SENTINEL, dtype=BF, device=DEV)
            vb = kb.clone()
            q = C.linear_qkv(a, wq[:, :K], bq, kb[1:-1], vb[1:-1], tslot, tpos, qs, kvs, hd, table, kind, splits, CNT)
            tagged(C, tag)
            assert gp.same_values(q, q_exp), f"q (rope {rope})"
            assert gp.bits_equal(kb, ek), f"K cache and its guards (rope {rope})"
            assert gp.bits_equal(vb, ev), f"V cache and its guards (rope {rope})"
    if direct and (kind == 0 or splits == 1):  # residual add in the kernel
        xb, xv = gp.guarded(D.x[:M, :N])
        assert C.linear_residual(a, ww, bias, xv, splits, kind, CNT, False) is None
        tagged(C, tag)
        eb, _ = gp.guarded((xe + yw + bias.double()[None, :]).float())
        assert gp.bits_equal(xb, eb), "residual and its guards"
    if splits > 1 or kind:  # slabs folded by the norm: fp32 (wide weights) and bf16
        for sbf, wt, yt in ((0, ww, yw), (1, w, y)):
            C.gemm_set_slab_bf16(sbf)
            xb, xv = gp.guarded(D.x[:M, :N])
            slab = C.linear_residual(a, wt, bias, xv, splits, kind, CNT, True)
            tagged(C, tag)
            assert slab is not None and slab.shape == (splits, M, N) and slab.dtype == (BF if sbf else torch.float32)
            assert gp.same_values(slab.double().sum(0), yt), f"slabs (bf16 {sbf})"
            fold(C, xv, slab, bias)
            eb, _ = gp.guarded((xe + yt + bias.double()[None, :]).float())
            assert gp.bits_equal(xb, eb), f"folded slabs and the guards (bf16 {sbf})"
    assert int(CNT.abs().sum()) == 0, "a ticket counter was left armed"


def run_point_probes(C, CNT, D, M, N, K, kind, splits, tag):
    """Placement (column code, k code) and poison at one shape of a variant."""
    for which in ("n", "k"):
        a, w, km, y = gp.placement_operands(M, N, K, which)
        if splits > 1 and not kind_combines(kind, tag):
            xv = torch.zeros(M, N, device=DEV)
            C.gemm_set_slab_bf16(0)
            fold(C, xv, C.linear_residual(dev(a), dev(w), None, xv, splits, kind, CNT, True), None)
            out = xv
        else:
            out = C.linear(dev(a), dev(w), None, 0, kind, splits, CNT)
        tagged(C, tag)
        msg = gp.placement_mismatch(out, y, which, km, N, K)
        assert msg is None, msg
    a, w, ww = (gp.poisoned(t[:r, :K].contiguous()) for t, r in ((D.a, M), (D.w, N), (D.ww, N)))
    assert a.stride(0) == K + 16 and a.data_ptr() % 16 == 0
    if splits > 1 and not kind_combines(kind, tag):
        C.gemm_set_slab_bf16(0)
        xv = torch.zeros(M, N, device=DEV)
        fold(C, xv, C.linear_residual(a, ww, None, xv, splits, kind, CNT, True), None)
        tagged(C, tag)
        assert gp.same_values(xv, D.y(K, True)[:M, :N]), "poison outside [M, K] / [N, K] reached a result"
    else:
        out = C.linear(a, w, D.bias[:N], 0, kind, splits, CNT)
        tagged(C, tag)
        assert gp.same_values(out, D.y(K)[:M, :N] + D.bias[:N].double()[None, :]), "poison reached a bf16 result"
        assert gp.same_values(C.linear_f32(a, ww, kind, splits, CNT), D.y(K, True)[:M, :N]), "poison reached an fp32 result"
    assert int(CNT.abs().sum()) == 0


def kind_combines(kind, tag):
    return kind != 1 or tag.startswith("ring8<2")


# ---------------------------------------------------------------------------
# gemm_sk (kind 0)
# ---------------------------------------------------------------------------
SK_K = (32, 64, 480, 512, 544, 1056, 1600)  # both sides of the 128 / 256 / 512-k rounds
# rows -> 16-row tiles per row block (MT) with 128-row blocks: every instantiated MT, and two row blocks
SK_MT128 = {1: 1, 16: 1, 17: 2, 33: 3, 49: 4, 65: 6, 97: 8, 128: 8, 129: 6, 200: 8, 256: 8}
SK_MT64 = {65: 3, 97: 4, 128: 4, 200: 4}    # the default 64-row blocks: 2, 2, 2 and 4 row blocks


def sk_splits(K):
    return [s for s in (1, 2, 3, 7) if s <= K // 32]


@pytest.mark.parametrize("nw", [1, 2])
@pytest.mark.parametrize("M,rows", [(m, 128) for m in SK_MT128] + [(m, 64) for m in SK_MT64])
def test_sk_every_epilogue(C, CNT, M, rows, nw):
    """gemm_sk: every MT and the row-block path, 64- and 128-column tiles (N =
    192: a masked half tile at NW 2), K on both sides of every round length,
    1 / 2 / 3 / 7 splits combined in the kernel and deferred as slabs."""
    RAN.append("test_sk_every_epilogue")
    D = data("sk")
    C.gemm_set_sk_rows(rows)
    C.gemm_set_nw2_rows(0 if nw == 2 else 1 << 30)
    mt = (SK_MT128 if rows == 128 else SK_MT64)[M]
    for K in SK_K:
        for splits in sk_splits(K):
            run_epilogues(C, CNT, D, "sk", M, 192, K, 0, splits, f"sk<{mt},{nw}>", silu_n=256, silu_tag=f"sk<{mt},2>")


@pytest.mark.parametrize("nw", [1, 2])
def test_sk_placement_and_poison(C, CNT, nw):
    C.gemm_set_nw2_rows(0 if nw == 2 else 1 << 30)
    run_point_probes(C, CNT, data("sk"), 97, 192, 544, 0, 3, f"sk<4,{nw}>")
    run_point_probes(C, CNT, data("sk"), 33, 192, 1056, 0, 1, f"sk<3,{nw}>")


# ---------------------------------------------------------------------------
# 128x128 tiled kernel and gemm_ring
# ---------------------------------------------------------------------------
TILED_M = (1, 95, 96, 97, 127, 128, 129, 257)
TILED_K = (64, 128, 192, 256, 640)  # 1, 2, 3, 4 and 10 k-steps: fewer than, equal to and more than the rings


def ring_knobs(C, variant):
    if variant == "tiled":
        return
    C.gemm_set_tiled3_max(1 << 30)
    slots, tn = {"ring<3,128>": (3, 128), "ring<4,128>": (4, 128), "ring<3,64>": (3, 64), "ring<3,32>": (3, 32),
                 "ring<3,64,m96>": (3, 64)}[variant]
    C.gemm_set_ring_slots(slots)
    C.gemm_set_ring_tn(tn)
    if variant == "ring<3,64,m96>":
        C.gemm_set_ring_m96(1 << 30)


def ring_tag(variant, M, N, splits):
    """The kernel launch_tiled picks under ring_knobs(variant): 32-wide tiles
    need N % 32 == 0 and 96-row tiles M > 128 and one split; both fall back to
    the 128x64 ring."""
    if variant == "ring<3,32>" and N % 32:
        return "ring<3,64>"
    if variant == "ring<3,64,m96>" and (M <= 128 or splits > 1):
        return "ring<3,64>"
    return variant


@pytest.mark.parametrize("N", [144, 352])  # a partial last tile at every tile width
@pytest.mark.parametrize("M", TILED_M)
@pytest.mark.parametrize("variant", ["tiled", "ring<3,128>", "ring<4,128>", "ring<3,64>", "ring<3,32>", "ring<3,64,m96>"])
def test_tiled_and_ring_every_epilogue(C, CNT, variant, M, N):
    RAN.append("test_tiled_and_ring_every_epilogue")
    D = data("tiled")
    ring_knobs(C, variant)
    for K in TILED_K:
        for splits in ((1, 2) if K >= 128 else (1,)):
            run_epilogues(C, CNT, D, variant, M, N, K, 1, splits, ring_tag(variant, M, N, splits), combine=False,
                          silu_tag=ring_tag(variant, M, N // 32 * 32, splits))  # SiLU runs on the first N // 32 * 32 rows


@pytest.mark.parametrize("variant", ["tiled", "ring<3,128>", "ring<4,128>", "ring<3,64>", "ring<3,32>", "ring<3,64,m96>"])
def test_tiled_and_ring_placement_and_poison(C, CNT, variant):
    ring_knobs(C, variant)
    run_point_probes(C, CNT, data("tiled"), 257, 352, 640, 1, 1, variant)
    run_point_probes(C, CNT, data("tiled"), 129, 352, 192, 1, 2, ring_tag(variant, 129, 352, 2))


# ---------------------------------------------------------------------------
# gemm_ring8
# ---------------------------------------------------------------------------
RING8 = {"var1": (1, 0, "ring8<1,3>"), "var2": (2, 0, "ring8<2,3>"), "var2-rot": (2, 1, "ring8<2,3>"),
         "var2-nt": (2, 2, "ring8<2,3,nt>"), "var2-bl": (2, 4, "ring8<2,3,bl>")}
RING8_K = (64, 192, 640, 1600)


def ring8_knobs(C, var, flags, pack=0):
    C.gemm_set_tiled3_max(1 << 30)
    C.gemm_set_ring_tn(64)
    C.gemm_set_ring8(var)
    C.gemm_set_ring8_flags(flags)
    C.gemm_set_ring8_pack(pack)


@pytest.mark.parametrize("N", [144, 352])
@pytest.mark.parametrize("M", TILED_M)
@pytest.mark.parametrize("variant", list(RING8))
def test_ring8_every_epilogue(C, CNT, variant, M, N):
    """8-wave 128x64 ring: both wave layouts, rotated K start, nt and
    buffer-load weight staging; the 8-computing-wave layout also combines 2 / 3
    / 4 splits in the kernel, the loader-wave layout writes slabs only."""
    var, flags, tag = RING8[variant]
    RAN.append("test_ring8_every_epilogue")
    D = data("ring8")
    ring8_knobs(C, var, flags)
    for K in RING8_K:
        for splits in [s for s in (1, 2, 3, 4) if s <= K // 64]:
            run_epilogues(C, CNT, D, "ring8", M, N, K, 1, splits, tag, combine=var == 2)


@pytest.mark.parametrize("variant", list(RING8))
def test_ring8_placement_and_poison(C, CNT, variant):
    var, flags, tag = RING8[variant]
    ring8_knobs(C, var, flags)
    run_point_probes(C, CNT, data("ring8"), 257, 352, 640, 1, 1, tag)
    run_point_probes(C, CNT, data("ring8"), 129, 352, 1600, 1, 3, tag)


def pack_w(w):  # [N / 64][K / 64][64][64], as tools/bench_ring8_pack.py
    N, K = w.shape
    return w.view(N // 64, 64, K // 64, 64).permute(0, 2, 1, 3).contiguous().view(N, K)


def pack_a(a):  # [K / 64][M][64]
    M, K = a.shape
    return a.view(M, K // 64, 64).permute(1, 0, 2).contiguous().view(M, K)


@pytest.mark.parametrize("N", [144, 352])
@pytest.mark.parametrize("M", TILED_M)
@pytest.mark.parametrize("pack", [1, 2, 3])
def test_ring8_packed_operands(C, CNT, pack, M, N):
    """k-block-packed operands (A/B variants of the 8-computing-wave ring):
    exact, hence bit-equal to the unpacked launch.  The packed weight is
    padded to whole 64-row blocks (the layout's unit; the kernel reads the
    last block's rows < N out of it)."""
    RAN.append("test_ring8_packed_operands")
    D = data("ring8")
    Np = (N + 63) // 64 * 64
    for K in RING8_K:
        a = D.a[:M, :K].contiguous()
        wpad = torch.zeros(Np, K, dtype=BF, device=DEV)
        wwpad = wpad.clone()
        wpad[:N], wwpad[:N] = D.w[:N, :K], D.ww[:N, :K]
        ap = pack_a(a) if pack & 2 else a
        wp = (pack_w(wpad) if pack & 1 else wpad)[:N]
        wwp = (pack_w(wwpad) if pack & 1 else wwpad)[:N]
        for splits in [s for s in (1, 3) if s <= K // 64]:
            ring8_knobs(C, 2, 0, 0)
            plain = C.linear(a, wpad[:N], D.bias[:N], 0, 1, splits, CNT)
            tagged(C, "ring8<2,3>")
            ring8_knobs(C, 2, 0, pack)
            out = C.linear(ap, wp, D.bias[:N], 0, 1, splits, CNT)
            tagged(C, f"ring8<2,3,pk{pack}>")
            assert gp.same_values(out, D.y(K)[:M, :N] + D.bias[:N].double()[None, :]) and torch.equal(out, plain)
            out = C.linear_f32(ap, wwp, 1, splits, CNT)
            tagged(C, f"ring8<2,3,pk{pack}>")
            assert gp.same_values(out, D.y(K, True)[:M, :N])
    assert int(CNT.abs().sum()) == 0


# ---------------------------------------------------------------------------
# gemm_big and gemm_p8 (256x256 tiles)
# ---------------------------------------------------------------------------
BIG_TAG = {0: "big", 1: "p8<0>", 4: "p8<4>"}


@pytest.mark.parametrize("N", [272, 320])   # a 16- and a 64-column tail in the second tile
@pytest.mark.parametrize("M", [256, 257, 511, 513])
@pytest.mark.parametrize("group", [0, 4])
@pytest.mark.parametrize("bk", [0, 1, 4])
def test_big_every_epilogue(C, CNT, bk, group, M, N):
    RAN.append("test_big_every_epilogue")
    D = data("big")
    C.gemm_set_big_min(1)
    C.gemm_set_big_kind(bk)
    C.gemm_set_big_group(group)
    for K in (64, 128, 256, 384, 640):
        for splits in ((1, 2) if K >= 128 else (1,)):
            run_epilogues(C, CNT, D, BIG_TAG[bk], M, N, K, 1, splits, BIG_TAG[bk], combine=False)


@pytest.mark.parametrize("bk", [0, 1, 4])
def test_big_placement_and_poison(C, CNT, bk):
    C.gemm_set_big_min(1)
    C.gemm_set_big_kind(bk)
    run_point_probes(C, CNT, data("big"), 513, 320, 640, 1, 1, BIG_TAG[bk])
    run_point_probes(C, CNT, data("big"), 257, 272, 384, 1, 2, BIG_TAG[bk])


# ---------------------------------------------------------------------------
# gemm_d256 (kinds 2 and 3)
# ---------------------------------------------------------------------------
def d256_tag(kind, slots, N):
    bn = 128 if kind == 3 and N % 128 == 0 else 64
    return f"d256<{bn},{min(slots, 3) if bn == 128 else slots}>"


@pytest.mark.parametrize("N", [352, 384])  # 352: a partial 64-wide tile, and 64-wide tiles under kind 3
@pytest.mark.parametrize("M", [1, 255, 256, 257, 513, 1024])
@pytest.mark.parametrize("slots", [2, 3, 4])
@pytest.mark.parametrize("kind", [2, 3])
def test_d256_every_epilogue(C, CNT, kind, slots, M, N):
    RAN.append("test_d256_every_epilogue")
    D = data("d256")
    C.gemm_set_d256_slots(slots)
    assert C.gemm_d256_bn(kind, M, N, 64) == (128 if kind == 3 and N == 384 else 64)
    for K in (64, 128, 192, 256, 320, 1600):
        for splits in [s for s in (1, 2, 3, 5) if s <= K // 64]:
            run_epilogues(C, CNT, D, "d256", M, N, K, kind, splits, d256_tag(kind, slots, N))


@pytest.mark.parametrize("kind,slots", [(2, 2), (2, 3), (2, 4), (3, 2), (3, 3)])
def test_d256_placement_and_poison(C, CNT, kind, slots):
    C.gemm_set_d256_slots(slots)
    run_point_probes(C, CNT, data("d256"), 513, 384, 320, kind, 1, d256_tag(kind, slots, 384))
    run_point_probes(C, CNT, data("d256"), 257, 384, 1600, kind, 3, d256_tag(kind, slots, 384))


# ---------------------------------------------------------------------------
# stale split-K state
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sk", "ring8", "d256"])
def test_split_k_ignores_stale_workspace(C, CNT, family):
    """A larger-valued problem first, then a different, smaller-valued shape
    on the same ticket counters: the workspace comes from torch.empty (the
    allocator hands the freed block back), so a partial that is read before it
    is written, or a ticket left over, changes the second, exact result."""
    D = data(family)
    kind = {"sk": 0, "ring8": 1, "d256": 2}[family]
    if family == "ring8":
        ring8_knobs(C, 2, 0)
    (M1, N1, K1, S1), (M2, N2, K2, S2) = {"sk": ((64, 256, 1600, 7), (33, 192, 544, 3)),
                                          "ring8": ((257, 352, 1600, 4), (129, 144, 640, 3)),
                                          "d256": ((513, 384, 1600, 5), (255, 352, 320, 3))}[family]
    for _ in range(2):
        big = C.linear_f32(D.a[:M1, :K1], D.ww[:N1, :K1], kind, S1, CNT)
        assert gp.same_values(big, D.y(K1, True)[:M1, :N1])
        del big
        out = C.linear(D.a[:M2, :K2], D.w[:N2, :K2], D.bias[:N2], 0, kind, S2, CNT)
        assert gp.same_values(out, D.y(K2)[:M2, :N2] + D.bias[:N2].double()[None, :])
        out = C.linear_f32(D.a[:M2, :K2], D.ww[:N2, :K2], kind, S2, CNT)
        assert gp.same_values(out, D.y(K2, True)[:M2, :N2])
        del out
    assert int(CNT.abs().sum()) == 0


# ---------------------------------------------------------------------------
# gemv
# ---------------------------------------------------------------------------
GEMV_K = (8, 504, 512, 520, 2048, 2056, 4096, 4104, 8192, 8200, 14336)  # every gv_nb bucket edge, the 512 chunk
_GEMV = {}


def gemv_data(K):
    if K not in _GEMV:
        a, w, bias, x = gp.integer_operands(8, 1008, K, seed=K)
        y = gp.exact_product(a, w)
        gp.assert_bf16_exact(y, bias)
        ww = gp.wide_weights(w, K)
        _GEMV[K] = SimpleNamespace(ai=a, wi=w, bi=bias, a=gp.poisoned(dev(a)), w=gp.poisoned(dev(w)),
                                   ww=gp.poisoned(dev(ww)), bias=dev(bias), x=dev(x, torch.float32),
                                   y=y.double().to(DEV), yw=gp.exact_product(a, ww).double().to(DEV), silu={})
    return _GEMV[K]


def gemv(C, x, w, bias, epi, norm=(0, None, None, 0.0), resid=None, qkv=None):
    kc, vc, tslot, tpos, qs, kvs, hd, rope = qkv or (None, None, None, None, 0, 0, 0, None)
    return C.gemv(x, w, bias, epi, *norm, resid, kc, vc, tslot, tpos, qs, kvs, hd, rope)


def gemv_qkv(C, x, w, bias, y_exact, M, N, norm=(0, None, None, 0.0)):
    """QKV epilogue of the GEMV without and with the synthetic RoPE: q, both
    caches and their guards.  w, bias: model order, [N, K] on the GPU."""
    qs, kvs, hd, nh, nkv = gp.qkv_dims(N)
    tslot, tpos, S = gp.token_map(M)
    for rope in (False, True):
        table = gp.rope_table_exact(S, hd) if rope else None
        perm = (gp.qkv_weight_order(N) if rope else torch.arange(N)).to(DEV)
        q_exp, ek, ev = gp.qkv_expected(y_exact, N, tslot, tpos, 3, S, table)
        kb = torch.full((5, nkv, S, hd), gp.SENTINEL, dtype=BF, device=DEV)
        vb = kb.clone()
        wq = gp.poisoned(w[perm].contiguous())
        q = gemv(C, x, wq, bias[perm].contiguous(), 6, norm,
                 qkv=(kb[1:-1], vb[1:-1], tslot.to(DEV), tpos.to(DEV), qs, kvs, hd, None if table is None else table.to(DEV)))
        assert gp.same_values(q, q_exp.to(DEV)), f"gemv q (rope {rope})"
        assert gp.bits_equal(kb, ek) and gp.bits_equal(vb, ev), f"gemv caches and guards (rope {rope})"


@pytest.mark.parametrize("K", GEMV_K)
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8])
def test_gemv_every_epilogue(C, M, K):
    """Plain (norm 0) GEMV: every epilogue at N = 1000 (a partial last
    workgroup) and 1008, both weight-load kinds; the operands are poisoned
    views, so the clamped tail chunks past K must meet the zero-padded LDS
    image and nothing else."""
    if not C.gemv_ok(M, K, 0, 0):
        pytest.skip("shape not on the GEMV")
    D = gemv_data(K)
    a = D.a[:M]
    for N in (1000, 1008):
        w, ww, bias = D.w[:N], D.ww[:N], D.bias[:N]
        y, yw = D.y[:M, :N], D.yw[:M, :N]
        yb = y + bias.double()[None, :]
        for nt in (0, 1):
            C.gemv_set_nt(nt)
            assert gp.same_values(gemv(C, a, w, bias, 0), yb), "gemv bf16 + bias"
            act_ok("gemv", gemv(C, a, w, bias, 1), "gelu", yb)
            out = gemv(C, a, ww, None, 3)
            assert out.dtype == torch.float32 and gp.same_values(out, yw), "gemv fp32"
            seg = torch.full((M, N // 8), float("nan"), device=DEV)
            out = C.gemv_logits(a, ww, 0, None, None, 0.0, seg)
            assert gp.same_values(out, yw) and gp.same_values(seg, gp.segmax_expected(yw)), "gemv logits + segmax"
            xb, xv = gp.guarded(D.x[:M, :N])
            assert gemv(C, a, ww, bias, 4, resid=xv) is None
            eb, _ = gp.guarded((D.x[:M, :N].double() + yw + bias.double()[None, :]).float())
            assert gp.bits_equal(xb, eb), "gemv residual and its guards"
            for which in ("up", "gate"):
                if which not in D.silu:
                    ai, wi, gate, up = gp.silu_operands(D.ai, D.wi[:992], which)
                    gp.assert_bf16_exact(up)
                    D.silu[which] = (gp.poisoned(dev(ai)), gp.poisoned(interleave_gate_up(dev(wi), 496).contiguous()),
                                     gate.double().to(DEV), up.double().to(DEV))
                ad, wd, gate, up = D.silu[which]
                out = gemv(C, ad[:M], wd, None, 2)
                if which == "up":
                    assert gp.same_values(out, 32 * up[:M]), "gemv silu(32) * up"
                else:
                    act_ok("gemv", out, "silu", gate[:M])
        C.gemv_set_nt(0)
        gemv_qkv(C, a, D.w[:N].contiguous(), bias, (y.cpu() + D.bi[:N][None, :]).long(), M, N)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("K", [504, 520, 768, 2048, 2056, 4096, 4104, 8192])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("rms", [False, True])
def test_gemv_fused_norm(C, rms, M, K, eps):
    """LayerNorm / RMSNorm in the GEMV's prologue on the balanced +-1 rows:
    the normalised bf16 row is exactly x gamma + beta, so every (epilogue,
    norm) pair lsd_gemv_ok lists gives an exact result."""
    code = 2 if rms else 1
    if not C.gemv_ok(M, K, 3, code):
        pytest.skip("shape not on the fused-norm GEMV")
    N = 1008
    x, gamma, beta, w, bias, y = gp.norm_case(M, N, K, rms, eps)
    gp.assert_bf16_exact(y, bias)
    xd = gp.poisoned(x.to(DEV))
    norm = (code, dev(gamma), None if rms else dev(beta), eps)
    wd, bd = gp.poisoned(dev(w)), dev(bias)
    yd = y.double().to(DEV)
    yb = yd + bd.double()[None, :]
    out = gemv(C, xd, wd, None, 3, norm)
    assert gp.same_values(out, yd), "fused norm, fp32"
    seg = torch.full((M, N // 8), float("nan"), device=DEV)
    out = C.gemv_logits(xd, wd, *norm, seg)
    assert gp.same_values(out, yd) and gp.same_values(seg, gp.segmax_expected(yd)), "fused norm, logits + segmax"
    gemv_qkv(C, xd, dev(w), bd, (y + bias[None, :]).long(), M, N, norm)
    if rms:
        assert C.gemv_ok(M, K, 2, 2)
        # the probes' pinned column: the normalised column 0 must be 1, so x[:, 0] = gamma[0] = 1; a row
        # that had -1 there hands one +1 back where gamma is 0 (its normalised value stays 0): still balanced
        x1, g1 = x.clone(), gamma.clone()
        g1[0] = 1
        x1[:, 0] = 1
        for r in range(M):
            if x[r, 0] != 1:
                x1[r, int(torch.nonzero((x[r, 1:] == 1) & (gamma[1:] == 0))[0]) + 1] = -1
        assert bool((x1.sum(1) == 0).all())
        xn1 = x1.long() * g1[None, :]
        for which in ("up", "gate"):
            _, ws, gate, up = gp.silu_operands(xn1, w[:992], which)
            gp.assert_bf16_exact(up)
            out = gemv(C, gp.poisoned(x1.to(DEV)), gp.poisoned(interleave_gate_up(dev(ws), 496).contiguous()), None, 2,
                       (2, dev(g1), None, eps))
            if which == "up":
                assert gp.same_values(out, 32 * up.double().to(DEV)), "fused RMSNorm, silu(32) * up"
            else:
                act_ok("gemv", out, "silu", gate.double().to(DEV))
    else:
        assert C.gemv_ok(M, K, 1, 1)
        act_ok("gemv", gemv(C, xd, wd, bd, 1, norm), "gelu", yb)


# ---------------------------------------------------------------------------
# routed launches: HipBackend at default routing
# ---------------------------------------------------------------------------
def tiled_tag(R, M, N, K, S):
    """launch_tiled's choice (gemm.hip) under HipBackend's knobs."""
    bm, bn = math.ceil(M / 256), math.ceil(N / 256)
    if M >= 256 and K % 64 == 0 and bm * bn * S >= R.big_min_blocks:
        return "p8<4>"
    tm, tn64 = math.ceil(M / 128), math.ceil(N / 64)
    if R.ring_tn in (0, 32, 64):
        narrow = R.ring_tn == 32 or (R.ring_tn == 0 and tm * tn64 * S < R.ring_fill)
        if narrow and N % 32 == 0 and tm * math.ceil(N / 32) * S <= 2 * R.tiled3_max:
            return "ring<3,32>"
        if tm * tn64 * S <= R.tiled3_max:
            return {0: "ring<3,64>", 1: "ring8<1,3>", 2: "ring8<2,3>"}[R.ring8]
    tn = math.ceil(N / 128)
    if tm * tn * S <= R.tiled3_max // 2:
        return f"ring<{R.ring_slots},128>"
    return "tiled"


def routed_tag(C, R, M, N, K, kind, S, epi=0):
    if kind is False or kind == 0:
        rb = C.gemm_sk_rblocks(M, N, S)
        mt = math.ceil(math.ceil(M / rb) / 16)
        return f"sk<{mt + 1 if mt in (5, 7) else mt},{C.gemm_sk_nw(M, epi)}>"
    if kind in (2, 3):
        return d256_tag(kind, R.d256_slots, N)
    return tiled_tag(R, M, N, K, S)


@pytest.mark.parametrize("N,K", [(384, 640), (384, 1280), (4160, 640)])  # K 1280 > tiled_short_k: split-K below 129 rows
@pytest.mark.parametrize("M", [8, 9, 64, 200, 256, 300])
def test_routed_launches_are_exact(C, M, N, K):
    """HipBackend().linear / linear_residual / logits / qkv_kv_append at the
    default routing: exact results, and the kernel Routing predicts (8 rows:
    the GEMV, which leaves the GEMM launch tag alone)."""
    from llm_sharding_demo_amd.ops import Residual
    from llm_sharding_demo_amd.ops.hip import HipBackend

    D = data("routed")
    be = HipBackend()
    R = be.R
    be.counters = torch.zeros(8 << 16, dtype=torch.int32, device=DEV)
    be.decode = True
    a, w, ww, bias = D.a[:M, :K].contiguous(), D.w[:N, :K].contiguous(), D.ww[:N, :K].contiguous(), D.bias[:N]
    y, yw = D.y(K)[:M, :N], D.y(K, True)[:M, :N]
    yb = y + bias.double()[None, :]
    C.linear(D.a[:1, :64], D.w[:64, :64], None, 0, 0, 1, None)  # a known tag to start from
    mark = C.gemm_last_launch()
    assert mark == "sk<1,1>"

    def expect(kind, S, epi=0):
        if M <= R.gemv_max_m:
            assert C.gemv_ok(M, K, epi, 0) and C.gemm_last_launch() == mark, "8 rows belong on the GEMV"
        else:
            tagged(C, routed_tag(C, R, M, N, K, kind, S, epi))

    kind, S = R.gemm_kw(M, N, K, 1, 1)
    assert gp.same_values(be.linear(a, w, bias), yb)
    expect(kind, S)
    act_ok("routed", be.linear(a, w, bias, "gelu"), "gelu", yb)
    expect(kind, S, 1)
    out = be.logits(a, ww)
    assert gp.same_values(out, yw)
    seg = getattr(out, "_lsd_segmax", None)
    assert seg is None or gp.same_values(seg, gp.segmax_expected(yw))
    expect(*R.logits_kw(M, N, K, 1), 3)
    # production slabs are bf16: exact on the bf16 probe's partials; fp32 slabs on the wide one
    for sbf, wt, yt in ((1, w, y), (0, ww, yw)):
        C.gemm_set_slab_bf16(sbf)
        xb, xv = gp.guarded(D.x[:M, :N])
        r = Residual(xv)
        be.linear_residual(a, wt, bias, r)
        expect(R.tiled(M, N), R.resid_splits(M, N, K, True, 1), 4)
        be.flush(r)
        eb, _ = gp.guarded((D.x[:M, :N].double() + yt + bias.double()[None, :]).float())
        assert gp.bits_equal(xb, eb), f"routed residual and its guards (bf16 slabs {sbf})"
    if N == 384:  # GPT-2-like heads of 64: 2 q heads, 2 kv heads
        qs, kvs, hd, nkv = 128, 128, 64, 2
        tslot, tpos, S_ = gp.token_map(M)
        for rope in (False, True):
            table = gp.rope_table_exact(S_, hd) if rope else None
            from llm_sharding_demo_amd.ops.hip import rope_pair_permutation
            perm = (torch.cat([rope_pair_permutation(2, hd), rope_pair_permutation(2, hd) + qs, torch.arange(256, 384)])
                    if rope else torch.arange(N)).to(DEV)
            be._rope = None if table is None else table.to(DEV)
            kb = torch.full((5, nkv, S_, hd), gp.SENTINEL, dtype=BF, device=DEV)
            vb = kb.clone()
            meta = SimpleNamespace(token_slots=tslot.to(DEV), token_pos=tpos.to(DEV))
            mcfg = SimpleNamespace(q_size=qs, kv_size=kvs, head_dim=hd)
            q = be.qkv_kv_append(a, w[perm].contiguous(), bias[perm].contiguous(), kb[1:-1], vb[1:-1], meta, mcfg)
            expect(kind, S, 6)
            yq = yb.cpu().long()
            hp = rope_pair_permutation(1, hd)
            qe = yq[:, :qs].reshape(M, 2, hd).double()
            ke = yq[:, qs:2 * qs].reshape(M, 2, hd).double()
            if rope:
                qe, ke = gp.rope_rotate(qe, tpos, table.double())[..., hp], gp.rope_rotate(ke, tpos, table.double())[..., hp]
            ek = torch.full((5, nkv, S_, hd), gp.SENTINEL, dtype=torch.float64)
            ev = ek.clone()
            ek[tslot.long() + 1, :, tpos.long()] = ke
            ev[tslot.long() + 1, :, tpos.long()] = yq[:, 2 * qs:].reshape(M, 2, hd).double()
            assert gp.same_values(q, qe.reshape(M, qs).to(DEV)), f"routed q (rope {rope})"
            assert gp.bits_equal(kb, ek.to(BF)) and gp.bits_equal(vb, ev.to(BF)), f"routed caches (rope {rope})"
    assert int(be.counters.abs().sum()) == 0


# ---------------------------------------------------------------------------
# hipBLASLt wrappers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", [512, 100])
def test_blaslt_wrappers_are_exact(C, M):
    D = data("blaslt")
    N, K = 320, 640
    a, w, ww, bias = D.a[:M].contiguous(), D.w, D.ww, D.bias
    y, yw = D.y(K)[:M], D.y(K, True)[:M]
    out = C.blaslt_linear(a, w, bias, 0, 0)
    if out is None:
        pytest.skip("hipBLASLt has no algorithm for this shape")
    assert gp.same_values(out, y + bias.double()[None, :])
    out = C.blaslt_f32(a, ww, 0)
    if out is None:
        pytest.skip("hipBLASLt has no fp32-output algorithm for this shape")
    assert out.dtype == torch.float32 and gp.same_values(out, yw)
    xb, xv = gp.guarded(D.x[:M])
    if not C.blaslt_residual(a, ww, bias, xv, 0):
        pytest.skip("hipBLASLt has no residual algorithm for this shape")
    eb, _ = gp.guarded((D.x[:M].double() + yw + bias.double()[None, :]).float())
    assert gp.bits_equal(xb, eb)


# ---------------------------------------------------------------------------
# what ran
# ---------------------------------------------------------------------------
EVERY_TAG = ({f"sk<{mt},{nw}>" for mt in (1, 2, 3, 4, 6, 8) for nw in (1, 2)}
             | {"tiled", "ring<3,128>", "ring<4,128>", "ring<3,64>", "ring<3,32>", "ring<3,64,m96>",
                "ring8<1,3>", "ring8<2,3>", "ring8<2,3,nt>", "ring8<2,3,bl>", "ring8<2,3,pk1>", "ring8<2,3,pk2>",
                "ring8<2,3,pk3>", "big", "p8<0>", "p8<4>",
                "d256<64,2>", "d256<64,3>", "d256<64,4>", "d256<128,2>", "d256<128,3>"})


def test_every_launch_branch_was_reached():
    """Runs last: the tests above reached every launch branch of launch_sk_nw,
    launch_d256_bn and launch_tiled (a deselected run proves nothing here)."""
    print("tags:", sorted(TAGS))
    print("activation error / bound:", {k: round(v, 3) for k, v in sorted(ACT_WORST.items())})
    n_variant = (2 * (len(SK_MT128) + len(SK_MT64)) + 6 * len(TILED_M) * 2 + (len(RING8) + 3) * len(TILED_M) * 2
                 + 3 * 2 * 4 * 2 + 2 * 3 * 6 * 2)
    if len(RAN) < n_variant:  # a run that deselected some of the variant tests
        return
    assert TAGS == EVERY_TAG, (sorted(EVERY_TAG - TAGS), sorted(TAGS - EVERY_TAG))
