"""The GEMM launch rules as three places held them before
csrc/kernels/gemm_plan.h: the launchers of gemm.hip (sk_rblocks / sk_mt / sk_nw,
d256_bn / launch_d256_bn, launch_tiled), the sizing query
lsd_gemm_ring8_tiles that repeated launch_tiled, and run_gemm of bindings.cpp
that sized counters and workspace from the queries.  Transcribed branch by
branch and checked once against that extension's own bindings
(gemm_ring8_tiles, gemm_d256_bn, gemm_sk_rblocks, gemm_sk_nw) over the sweep of
tests/test_gemm_plan.py; plan_gemm() must reproduce it."""

DEFAULTS = dict(big_min_blocks=160, big_group=4, big_kind=4, tiled3_max_blocks=0, ring_slots=3, ring_tn=128,
                ring_fill=128, ring_m96=0, ring8=0, ring8_flags=0, ring8_pack=0, d256_slots=3, sk_rows=64,
                rb_fill=192, nw2_rows=1 << 30)
SILU_MUL, SLAB = 2, 5
# the lsd_gemm_set_* clamping (knobs without an entry are stored as given)
CLAMP = dict(big_group=lambda v: max(v, 0), big_kind=lambda v: v if v in (1, 4) else 0,
             ring_slots=lambda v: 4 if v == 4 else 3, ring_tn=lambda v: v if v in (0, 32, 64) else 128,
             ring8=lambda v: v if v in (1, 2) else 0, ring8_flags=lambda v: v & 7, ring8_pack=lambda v: v & 3,
             d256_slots=lambda v: min(max(v, 2), 4), sk_rows=lambda v: min(max(v, 16), 128))


def knobs(**kw):
    return dict(DEFAULTS, **{k: CLAMP.get(k, int)(v) for k, v in kw.items()})


def cdiv(a, b):
    return (a + b - 1) // b


def sk_rblocks(k, M, N, S):
    need = cdiv(M, 128)
    if M <= k["sk_rows"] or (N // 64) * S >= k["rb_fill"]:
        return need
    return max(cdiv(M, k["sk_rows"]), need)


def sk_mt(M, rb):
    mt = cdiv(cdiv(M, rb), 16)
    return mt + 1 if mt in (5, 7) else mt


def sk_nw(k, M, epi):
    return 2 if epi == SILU_MUL or M > k["nw2_rows"] else 1


def d256_bn(kind, M, N, K):
    if kind < 2 or M < 1 or M > 1024 or K % 64:
        return 0
    return 128 if kind == 3 and N % 128 == 0 else 64


def ring8_tiles(k, M, N, K, S):
    """lsd_gemm_ring8_tiles: the sizing copy of launch_tiled."""
    if k["ring8"] != 2:
        return 0
    if M >= 256 and K % 64 == 0 and cdiv(M, 256) * cdiv(N, 256) * S >= k["big_min_blocks"]:
        return 0
    if k["ring_tn"] not in (0, 32, 64):
        return 0
    tm, tn64 = cdiv(M, 128), cdiv(N, 64)
    narrow = k["ring_tn"] == 32 or (k["ring_tn"] == 0 and tm * tn64 * S < k["ring_fill"])
    if narrow and N % 32 == 0 and tm * cdiv(N, 32) * S <= 2 * k["tiled3_max_blocks"]:
        return 0
    if S == 1 and M > 128 and k["ring_m96"] > 0 and cdiv(M, 96) * tn64 <= k["ring_m96"]:
        return 0
    return tm * tn64 if tm * tn64 * S <= k["tiled3_max_blocks"] else 0


def launch_tiled(k, M, N, K, S, combine):
    """(tag, workgroups, block) or None where launch_tiled refused."""
    bm, bn = cdiv(M, 256), cdiv(N, 256)
    if M >= 256 and K % 64 == 0 and bm * bn * S >= k["big_min_blocks"]:
        return {1: "p8<0>", 4: "p8<4>"}.get(k["big_kind"], "big"), bm * bn * S, 512
    tm = cdiv(M, 128)
    if k["ring_tn"] in (0, 32, 64):
        tn64 = cdiv(N, 64)
        narrow = k["ring_tn"] == 32 or (k["ring_tn"] == 0 and tm * tn64 * S < k["ring_fill"])
        if narrow and N % 32 == 0 and tm * cdiv(N, 32) * S <= 2 * k["tiled3_max_blocks"]:
            return "ring<3,32>", tm * cdiv(N, 32) * S, 256
        if S == 1 and M > 128 and k["ring_m96"] > 0 and cdiv(M, 96) * tn64 <= k["ring_m96"]:
            return "ring<3,64,m96>", cdiv(M, 96) * tn64, 256
        if tm * tn64 * S <= k["tiled3_max_blocks"]:
            r8, fl, pk = k["ring8"], k["ring8_flags"], k["ring8_pack"]
            if combine and r8 != 2:
                return None
            if r8 == 1:
                return "ring8<1,3>", tm * tn64 * S, 512
            if r8 == 2:
                sfx = f",pk{pk}" if pk else ",bl" if fl & 4 else ",nt" if fl & 2 else ""
                return f"ring8<2,3{sfx}>", tm * tn64 * S, 512
            return "ring<3,64>", tm * tn64 * S, 256
    wgs = tm * cdiv(N, 128) * S
    if wgs <= k["tiled3_max_blocks"] // 2:
        return ("ring<4,128>" if k["ring_slots"] == 4 else "ring<3,128>"), wgs, 256
    return "tiled", wgs, 256


INVALID = (0, "", (1, 1, 1), 0, 0, 0)


def plan(k, M, N, K, S, epi, kind):
    """(valid, tag, grid, block, combine_tiles, tile_floats): the launch lsd_gemm
    made and the counters / workspace floats per tile and split run_gemm sized."""
    if not 0 <= epi <= 6 or min(M, N, K, S) < 1:  # the second: shapes run_gemm never passed on
        return INVALID
    combine = S > 1 and epi != SLAB
    if kind >= 2:
        bn = d256_bn(kind, M, N, K)
        if bn == 0:
            return INVALID
        slots = min(k["d256_slots"], 3) if bn == 128 else k["d256_slots"]
        tiles = cdiv(N, bn) * cdiv(M, 256)
        return (1, f"d256<{bn},{slots}>", (tiles * S, 1, 1), 512) + ((tiles, 256 * bn) if combine else (0, 0))
    if kind:
        t = launch_tiled(k, M, N, K, S, combine)
        if t is None:
            return INVALID
        r8 = ring8_tiles(k, M, N, K, S) if combine else 0
        return (1, t[0], (t[1], 1, 1), t[2]) + ((r8, 128 * 64) if r8 else (0, 0))
    rb = sk_rblocks(k, M, N, S)
    mt, nw = sk_mt(M, rb), sk_nw(k, M, epi)
    if mt not in (1, 2, 3, 4, 6, 8):
        return INVALID
    cols = cdiv(N, 64 * nw)
    return (1, f"sk<{mt},{nw}>", (cols, S, rb), 256) + ((cols * rb, mt * 16 * 64 * nw) if combine else (0, 0))
