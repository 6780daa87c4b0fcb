"""Constructed int8 operands and scales for the attention kernels, their fp64 reference and a DERIVED error bound.

CPU only: nothing here imports the HIP library.  tests/test_constructed_cases.py proves on the CPU that the bound is sound
(the oracle's restatement of the kernel stays inside it) and that it has teeth (a restatement with one deliberate mistake
leaves it); tests/test_constructed_logits_gpu.py holds the kernels to it.

Every case is a dict (``case(family, variant, D, N, causal, gran)``):
  q8 [1,2,M,D] / k8 [1,1,N,D] int8; q_scale [1,2,Gq] / k_scale [1,1,Gk] fp32 in the compact layout of the granularity
  ``gran`` (oracle.sage_oracle.gid_*); q_scale_rows [1,2,M] / k_scale_cols [1,1,N] their expansions; logit_mult and the
  sm_scale that produces it; causal; v_f16 / v_bf16 [1,1,N,D]; v_f8t [1,1,D,ceil64(N)] e4m3 (tokens in NATURAL order: the
  GPU test applies quant.fp8_token_order()) with v_scale [1,1,D].
Non-causal cases have M = 150 query rows (one full 128-row q-block, one wave with 22 valid rows, waves with none);
causal cases M = N.  GQA group 2.

All scales, and logit_mult, are powers of two, so the base-2 logit of (row m, key n) is the INTEGER score S[m,n] times a
power of two: exact in fp32 and in fp64, and the same number whichever way a kernel associates the three factors.
"""
import math

import numpy as np
import torch

from oracle import sage_oracle as O

B, HQ, HK = 1, 2, 1
M_FULL = 150
LOOP_NS = (320, 384, 456, 512)  # n_fast = 4, 5, 6, 7: four-slot ring exact/+1/+2/+3, two-slot ring even/odd, ragged 456
N_ONE = 456                     # families that do not depend on the loop shape
GRANS = ("per_block", "per_warp", "per_thread")
PVS = ("fp16", "bf16", "fp8")

K_LOG2E = float(np.float32(1.4426950408889634))  # csrc/sage_common.h kLog2e
BIAS = 12582912.0                                # csrc/sage_attn_body.h kBiasF (1.5 * 2^23)
LAZY_THR = {"fp16": 6.0, "bf16": 6.0, "fp8": 3.0}  # kLazyThr
FP8_OFFSET = 8.807                               # p carries 2^(8.807 - 3) under FP8 PV (kPOff)
P_BITS = {"fp16": 11, "bf16": 8, "fp8": 4}       # significand bits of P (implicit bit included)
OUT_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp8": torch.float16}


def _pow2_logit_mult(exp=-3):
    """(sm_scale, logit_mult) with logit_mult = fp32(sm_scale) * fp32(kLog2e) == 2^exp EXACTLY in fp32: the kernels
    compute ``sm_scale * kLog2e`` in fp32 (sage_attn.hip), so such an sm_scale makes logit_mult a power of two."""
    target = np.float32(2.0 ** exp)
    x = np.float32(2.0 ** exp / 1.4426950408889634)
    for cand in (x, np.nextafter(x, np.float32(1)), np.nextafter(x, np.float32(0))):
        if np.float32(cand) * np.float32(K_LOG2E) == target:
            return float(cand), float(target)
    raise AssertionError("no fp32 sm_scale gives a power-of-two logit_mult")


SM_SCALE, LOGIT_MULT = _pow2_logit_mult(-3)


def _u(D):
    """fixed +-1 vector"""
    g = torch.Generator().manual_seed(1234 + D)
    return (torch.randint(0, 2, (D,), generator=g) * 2 - 1).to(torch.int32)


def _gid_q(M, gran):
    if gran == "per_block":
        return O.gid_per_block(M, 128)
    if gran == "per_warp":
        return O.gid_per_warp_q(M, 128, 32)
    return O.gid_per_thread_q(M, 128, 32)


def _gid_k(N, gran):
    return O.gid_per_thread_k(N) if gran == "per_thread" else O.gid_per_block(N, 64)


def _uniform_scales(M, N, gran, q_exp, k_exp):
    _, gq = _gid_q(M, gran)
    _, gk = _gid_k(N, gran)
    return torch.full((B, HQ, gq), 2.0 ** q_exp), torch.full((B, HK, gk), 2.0 ** k_exp)


def _ladder_scales(M, N, gran, q_top_exp):
    """Q: exponent q_top_exp - ((3 g + h) % 4) for group g of head h (neighbouring groups always differ);
    K: exponent ((3 g + 5 tile) % 7) - 3 in -3..3 per per-thread group g of a tile (per_block / per_warp: one per tile,
    (5 tile) % 7 - 3): neighbouring groups and neighbouring tiles always differ."""
    _, gq = _gid_q(M, gran)
    _, gk = _gid_k(N, gran)
    g = torch.arange(gq).view(1, 1, gq)
    h = torch.arange(HQ).view(1, HQ, 1)
    qs = torch.pow(2.0, (q_top_exp - ((3 * g + h) % 4)).float())
    kg = torch.arange(gk)
    if gran == "per_thread":
        ke = (3 * (kg % 4) + 5 * (kg // 4)) % 7 - 3
    else:
        ke = (5 * kg) % 7 - 3
    ks = torch.pow(2.0, ke.float()).view(1, 1, gk).expand(B, HK, gk).contiguous()
    return qs.contiguous(), ks


def _v_normal(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, HK, N, D, generator=g)
    return v


def _v_triple(v):
    """fp16, bf16 and e4m3 V^T (+ v_scale) of one real V."""
    v16 = v.to(torch.float16)
    v8t, vsc, _ = O.per_channel_fp8(v16, "HND", smooth_v=False)
    return dict(v_f16=v16, v_bf16=v.to(torch.bfloat16), v_f8t=v8t, v_scale=vsc)


def _v_big(N, D):
    """fp16 |v| in [1e4, 6e4] with alternating signs; bf16 the same pattern up to 2^16; e4m3 codes of magnitude
    256..448 (448 on every fourth key) with v_scale on the power-of-two ladder 2^(d % 7 - 3) over channels."""
    g = torch.Generator().manual_seed(77)
    sign = 1.0 - 2.0 * ((torch.arange(N).view(N, 1) + torch.arange(D).view(1, D)) % 2)
    mag = 1.0e4 + 5.0e4 * torch.rand(N, D, generator=g)
    mag[::4] = 6.0e4
    v16 = (sign * mag).view(B, HK, N, D).to(torch.float16)
    vbf = (sign * mag * (65536.0 / 6.0e4)).view(B, HK, N, D).to(torch.bfloat16)
    codes = torch.tensor([448.0, 256.0, 320.0, 416.0])[torch.arange(N) % 4].view(N, 1) * sign  # all exact in e4m3
    npad = O.cdiv(N, 64) * 64
    v8t = torch.zeros(B, HK, D, npad)
    v8t[..., :N] = codes.t()
    vsc = torch.pow(2.0, (torch.arange(D) % 7 - 3).float()).view(B, HK, D).contiguous()
    return dict(v_f16=v16, v_bf16=vbf, v_f8t=v8t.to(torch.float8_e4m3fn), v_scale=vsc)


def regran(c, gran):
    """The same case with its (uniform) scales laid out for another granularity: the logits do not change, so the copy
    shares the cached reference."""
    assert c["family"] in ("ramp", "extreme_s", "one_hot")
    d = dict(c)
    _, gq = _gid_q(c["M"], gran)
    _, gk = _gid_k(c["N"], gran)
    d["q_scale"] = c["q_scale"][..., :1].expand(B, HQ, gq).contiguous()
    d["k_scale"] = c["k_scale"][..., :1].expand(B, HK, gk).contiguous()
    d["gran"] = gran
    assert torch.equal(O.expand_q_scale(d["q_scale"], c["M"], gran), c["q_scale_rows"])
    return d


def _finish(c, M, N, gran):
    c["_cache"] = {}
    c["q_scale_rows"] = O.expand_q_scale(c["q_scale"], M, gran)
    c["k_scale_cols"] = O.expand_k_scale(c["k_scale"], N, gran)
    c.update(M=M, N=N, gran=gran, logit_mult=LOGIT_MULT, sm_scale=SM_SCALE)
    assert c["q8"].dtype == torch.int8 and c["k8"].dtype == torch.int8
    return c


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------

def _ladder_operands(D, N, M, gran, q_top_exp):
    gq = torch.Generator().manual_seed(100 + D)
    q8 = torch.randint(-127, 128, (B, HQ, 512, D), generator=gq)[:, :, :M].to(torch.int8)
    gk = torch.Generator().manual_seed(200 + D)
    k_real = 48.0 * torch.randn(B, HK, 512, D, generator=gk)[:, :, :N]
    qs, ks = _ladder_scales(M, N, gran, q_top_exp)
    kcols = O.expand_k_scale(ks, N, gran)
    k8 = torch.round(k_real / kcols.unsqueeze(-1)).clamp(-127, 127).to(torch.int8)
    return dict(q8=q8.contiguous(), k8=k8.contiguous(), q_scale=qs, k_scale=ks)


def scale_ladder(D, N, causal, gran, lsb_exp=-12, big_v=False):
    """A seeded real K (sigma 48) quantized with hand-chosen power-of-two scales 2^-3..2^3, permuted over the per-thread key
    groups and over the tiles (coarse scales use a few integer levels, fine ones clamp at +-127); uniform int8 Q with
    per-row-group scales on a ladder of four exponents.  The LARGEST LSB of any row, q_scale * logit_mult * 2^3, is
    2^lsb_exp: -12 for the ordinary family, -6 / -5 / -4 for ``coarse_lsb``."""
    M = N if causal else M_FULL
    c = _ladder_operands(D, N, M, gran, lsb_exp)  # top q_scale 2^lsb_exp: times logit_mult 2^-3 and the top k_scale 2^3
    c.update(_v_big(N, D) if big_v else _v_triple(_v_normal(N, D, 300 + D)))
    c.update(family="big_v" if big_v else ("scale_ladder" if lsb_exp == -12 else "coarse_lsb"), causal=causal, D=D)
    return _finish(c, M, N, gran)


RAMP_UNITS = {  # step of the steepest row's per-tile maximum, in units of 2^-10 (base-2 logits)
    "0.5": 512, "6-": 6 * 1024 - 1, "6": 6 * 1024, "6+": 6 * 1024 + 1, "3-": 3 * 1024 - 1, "3": 3 * 1024,
    "3+": 3 * 1024 + 1, "40": 40 * 1024}
RAMP_R = (4, -4, 2, -2, 1, -1, 0)  # r_m cycles with period 7: every 32-row wave holds every trend, both signs
RAMP_SHAPES = ("ascending", "descending", "sawtooth")


def ramp_steps(pv):
    t = "6" if pv != "fp8" else "3"
    return ("0.5", t + "-", t, t + "+", "40")


def _ramp_levels(shape, ntiles):
    if shape == "ascending":
        lv = list(range(ntiles))
    elif shape == "descending":
        lv = list(range(ntiles - 1, -1, -1))
    else:  # 0 1 0 2 1 3 2 4: the maximum grows by one step on every odd tile, a tile two steps below it follows
        lv = [(j + 1) // 2 if j % 2 else max(j // 2 - 1, 0) for j in range(ntiles)]
    return [x - 3 for x in lv]  # centred so that |K| stays inside the digits' range


def ramp(D, N, causal, gran, step="6", shape="ascending"):
    """Rank-one integer scores S[m,n] = r_m * K_n, known in closed form.

    q8[m,:] = r_m * w * u and k8[n,:] = digits(K_n) * u with u a fixed +-1 vector and w = (1, 31, 31, ..., 31), so that
    q.k = r_m * (digit_0 + 31 * sum(other digits)) = r_m * K_n for ANY integer |K_n| <= 31*127*(D-1): the plain form
    r_m*u, c_n*u reaches only products of two int8, and the steps thr -+ 2^-10 need the 13-bit primes 6143 / 3071 (and
    5*1229, 7*439) as a factor.  K_n is a staircase over the 64-key tiles, K = level(tile) * units, r_m cycles through
    (4,-4,2,-2,1,-1,0) inside every wave.  With q_scale * k_scale * logit_mult = 2^-12 the steepest rows (r = 4) see their
    tile maximum move by exactly units * 2^-10 per level."""
    M = N if causal else M_FULL
    units = RAMP_UNITS[step]
    u = _u(D)
    w = torch.full((D,), 31, dtype=torch.int32)
    w[0] = 1
    r = torch.tensor([RAMP_R[m % 7] for m in range(M)], dtype=torch.int32)
    q8 = (r.view(M, 1) * (w * u).view(1, D)).view(1, 1, M, D).expand(B, HQ, M, D)
    ntiles = O.cdiv(N, 64)
    K = torch.tensor(_ramp_levels(shape, ntiles), dtype=torch.int64).repeat_interleave(64)[:N] * units
    A = torch.round(K.double() / 31).to(torch.int64)
    rem = K - 31 * A
    base = torch.div(A, D - 1, rounding_mode="floor")
    extra = A - base * (D - 1)  # 0 .. D-2
    dig = base.view(N, 1) + (torch.arange(D - 1).view(1, D - 1) < extra.view(N, 1)).to(torch.int64)
    digits = torch.cat([rem.view(N, 1), dig], dim=1)
    assert digits.abs().max() <= 127 and (q8.abs().max() <= 127)
    k8 = (digits.to(torch.int32) * u.view(1, D)).view(B, HK, N, D)
    qs, ks = _uniform_scales(M, N, gran, -5, -4)  # 2^-5 * 2^-4 * 2^-3 = 2^-12
    c = dict(q8=q8.to(torch.int8).contiguous(), k8=k8.to(torch.int8).contiguous(), q_scale=qs, k_scale=ks,
             family="ramp", causal=causal, D=D, r=r, K=K, units=units)
    c.update(_v_triple(_v_normal(N, D, 400 + D)))
    return _finish(c, M, N, gran)


def extreme_s(D, N, causal, gran, variant="corner"):
    """corner: every q8 = -128, k8 alternating -128 / 127 by key: S = +D*2^14 (2^21 at head_dim 128, the largest score the
    int8 format can produce) and -D*128*127 side by side in one tile; the scale product 2^-18 (2^-17 at head_dim 64) makes
    the logit spread 15.9.  zero: q8 = 0 and random k8: uniform weights, o = mean of V, lse2 = log2(keys)."""
    M = N if causal else M_FULL
    if variant == "corner":
        q8 = torch.full((B, HQ, M, D), -128, dtype=torch.int8)
        kv = torch.where(torch.arange(N) % 2 == 0, -128, 127).view(1, 1, N, 1).expand(B, HK, N, D)
        k8 = kv.to(torch.int8).contiguous()
        qs, ks = _uniform_scales(M, N, gran, -8 if D == 128 else -7, -7)  # * 2^-3 -> 2^-18 / 2^-17
    else:
        q8 = torch.zeros(B, HQ, M, D, dtype=torch.int8)
        k8 = torch.randint(-127, 128, (B, HK, N, D), generator=torch.Generator().manual_seed(500 + D)).to(torch.int8)
        qs, ks = _uniform_scales(M, N, gran, -5, -4)
    c = dict(q8=q8, k8=k8, q_scale=qs, k_scale=ks, family="extreme_s", variant=variant, causal=causal, D=D)
    c.update(_v_triple(_v_normal(N, D, 600 + D)))
    return _finish(c, M, N, gran)


ONE_HOT_KEYS = ("first", "63", "ragged", "last")


def one_hot_key(N, where):
    return {"first": 0, "63": 63, "ragged": 64 * (N // 64), "last": N - 1}[where]


def one_hot(D, N, causal, gran, where="last", subnormal=False):
    """Rank-one r_m*u, c_n*u with one key far ahead.  Ordinary: c_hot = 127, the others in -2..2, r_m in 40..127, LSB 2^-12:
    the lead D*r_m*(127-2)*2^-12 is >= 78 (base 2).  subnormal: the others are c = 0, c_hot = 4096/D and r_m cycles through
    15..24, so every other key has p = 2^-r_m relative to the hot one: inside fp16's subnormal range (2^-15..2^-24)."""
    M = N if causal else M_FULL
    u = _u(D)
    hot = one_hot_key(N, where)
    if subnormal:
        r = torch.tensor([15 + m % 10 for m in range(M)], dtype=torch.int32)
        cn = torch.zeros(N, dtype=torch.int32)
        cn[hot] = 4096 // D
    else:
        r = torch.tensor([40 + (m * 37) % 88 for m in range(M)], dtype=torch.int32)
        cn = torch.randint(-2, 3, (N,), generator=torch.Generator().manual_seed(700)).to(torch.int32)
        cn[hot] = 127
    q8 = (r.view(M, 1) * u.view(1, D)).view(1, 1, M, D).expand(B, HQ, M, D).to(torch.int8).contiguous()
    k8 = (cn.view(N, 1) * u.view(1, D)).view(B, HK, N, D).to(torch.int8).contiguous()
    qs, ks = _uniform_scales(M, N, gran, -5, -4)
    c = dict(q8=q8, k8=k8, q_scale=qs, k_scale=ks, family="one_hot", causal=causal, D=D, hot=hot, r=r, cn=cn,
             subnormal=subnormal)
    c.update(_v_triple(_v_normal(N, D, 800 + D)))
    return _finish(c, M, N, gran)


def coarse_lsb(D, N, causal, gran, lsb_exp=-6):
    return scale_ladder(D, N, causal, gran, lsb_exp=lsb_exp)


def big_v(D, N, causal, gran):
    return scale_ladder(D, N, causal, gran, big_v=True)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------------------------------

def scores(c):
    """exact integer scores [1,Hq,M,N] as float64 (|S| <= 2^21)"""
    g = HQ // HK
    return c["q8"].double() @ c["k8"].double().repeat_interleave(g, dim=1).transpose(2, 3)


def scale_matrix(c, q_rows=None, k_cols=None):
    """fp32 q_scale*logit_mult times k_scale as the kernels form it (body.h: qsc = q_scale * logit_mult, sc = qsc * k), in
    float64.  With the power-of-two scales of this file every product is exact."""
    q_rows = c["q_scale_rows"] if q_rows is None else q_rows
    k_cols = c["k_scale_cols"] if k_cols is None else k_cols
    qsc = q_rows * torch.tensor(c["logit_mult"], dtype=torch.float32)
    sc = qsc.unsqueeze(-1) * k_cols.repeat_interleave(HQ // HK, dim=1).unsqueeze(2)
    return sc.double()


def allowed(c, M=None, N=None):
    M, N = c["M"] if M is None else M, c["N"] if N is None else N
    if c["causal"]:
        return (torch.arange(N).view(1, 1, 1, N) <= torch.arange(M).view(1, 1, M, 1))
    return torch.ones(1, 1, M, N, dtype=torch.bool)


def v64(c, pv):
    """the V a kernel multiplies, dequantised, float64 [1,Hq,N,D]"""
    if pv == "fp16":
        v = c["v_f16"].double()
    elif pv == "bf16":
        v = c["v_bf16"].double()
    else:
        v = (c["v_f8t"].float().double()[..., :c["N"]] * c["v_scale"].double().unsqueeze(-1)).transpose(2, 3)
    return v.repeat_interleave(HQ // HK, dim=1)


def reference64(c, pv):
    """fp64 softmax (base 2) of the dequantised integers times the dequantised V.
    -> dict(o [1,Hq,M,D], lse2 [1,Hq,M], W normalised weights [1,Hq,M,N], wabsv = W @ |V|, sumabsv = sum_j |V_jd| over the
    keys the row attends)."""
    key, cache = ("ref", pv), c.setdefault("_cache", {})
    if key in cache:
        return cache[key]
    t = scores(c) * scale_matrix(c)
    ok = allowed(c)
    t = t.masked_fill(~ok, float("-inf"))
    m = t.amax(-1, keepdim=True)
    p = torch.exp2(t - m)
    l = p.sum(-1, keepdim=True)
    W = p / l
    V = v64(c, pv)
    out = dict(o=W @ V, lse2=(m + torch.log2(l)).squeeze(-1), W=W, wabsv=W @ V.abs(),
               sumabsv=ok.double().expand(1, HQ, -1, -1) @ V.abs())
    cache[key] = out
    return out


def _ulp(x, mant, emin):
    e = torch.floor(torch.log2(x.abs())).clamp(min=emin)
    return torch.exp2(e - mant)


def out_ulp(x, pv, dtype=None):
    """spacing of the output dtype at |x| (fp16 for fp16 / fp8 PV, bf16 for bf16 PV), subnormal floor included"""
    return _ulp(x, 10, -14) if (dtype or OUT_DTYPE[pv]) == torch.float16 else _ulp(x, 7, -126)


def row_lsb(c):
    """largest LSB of each row: max over the attended keys of q_scale * logit_mult * k_scale, [1,Hq,M] float64"""
    sc = scale_matrix(c).masked_fill(~allowed(c), 0.0)
    return sc.amax(-1)


def bound(c, pv, D=None, delta_zero=False):
    """Per-element tolerance of a kernel's (o, lse2) against reference64 -> (o_bound [1,Hq,M,D], lse_bound [1,Hq,M]).

    Every number is a format width or a constant of csrc/sage_attn_body.h:

      |o - o64|       <= (2 * 2^-t + (2^(2 delta) - 1) + 2^-18) * (W @ |V|)  +  sub  +  2 output ulps of |o64|
      |lse2 - lse2_64| <= [log2(1 + 2^-11) if D = 64 and fp16 P] + delta + 1.4427 * N * 2^-24 + 2 fp32 ulps of |lse2_64|

    * 2^-t, t = 11 / 8 / 4 significand bits of P in fp16 / bf16 / e4m3: one RNE rounding of every p is within 2^-t
      relative of it (half an ulp of a t-bit significand is at most 2^-t of the value).  A second 2^-t because the FP16-PV
      kernel at head_dim 64 divides by the sum of the ROUNDED P (row-sum MFMA): numerator and denominator each move by
      2^-t relative.  (For e4m3 this is the hard form 2^-3 of tests/test_fp8_derived_bound.py; its 6-sigma form assumes
      many comparable keys and does not hold for rows that a few keys dominate.)
    * delta = (12582912 + Smax) * 2^-24 * s with s the row's largest LSB and Smax the largest |S| of the case.  The
      kernel evaluates p = exp2(fma(as_float(bias + S), sc, c0)) with c0 = fma(-12582912, sc, kPOff - m_run), m_run the
      logit of some score: |c0| <= (12582912 + Smax) * sc (+ kPOff) and its rounding is half an ulp, 2^-24 |c0|.  One
      tile's exponent is therefore off by up to delta, the same for all its keys, and two tiles may err in opposite
      directions: weights move by 2^(2 delta) - 1 relative to each other.  At Smax = 2^21 delta is 0.875 s, not the
      0.75 s the comments in the kernel and in tests/conftest.py state (0.75 is its value for Smax << 12582912).
      FP8 PV adds the rounding of (kPOff - m_run) itself, which is exact only for kPOff = 0: half an ulp of at most
      Smax * s + 8.807, i.e. 2^-24 * (Smax * s + 8.807) more.
    * 2^-18 covers v_exp_f32 (1 ulp, 2^-23), the rounding of the fma result (|exponent| <= 31 for any p that survives
      fp16: 2^-24 * 31 * ln 2) and the fp32 accumulation over <= 512 keys.
    * sub, the subnormal floor of P: an fp16 P below 2^-14 is rounded to a multiple of 2^-24, off by <= 2^-25 absolute,
      while the row's largest p is >= 1 so l >= 1: 2^-25 * sum_j |V_jd| over the row's keys.  bf16 has fp32's exponent
      range: 0.  e4m3: half the subnormal spacing 2^-9 is 2^-10, and the row's largest p is at least 2^(8.807 - 3) (the
      running maximum lags the true one by at most kLazyThr = 3): 2^-10 * 2^-5.807 * sum_j |V_jd|.
    * 2 output ulps: the final rounding to fp16 / bf16 is half an ulp; the second guards the ulp boundary between o and
      o64.
    LSE: log2(1 + 2^-11) is the relative error of a sum of fp16-rounded P (conftest.LSE2_TOL_ROUNDED_P's first term);
    delta moves l by 2^(+-delta); N fp32 additions of positive terms each lose <= 2^-24 relative, log2(e) * N * 2^-24 in
    the logarithm (v_log_f32's own ulp is inside the 2 fp32 ulps).
    ``delta_zero``: for operands whose logits are all equal on a row no relative movement between tiles can change the
    weights' ratios -- used by the degenerate-input operator tests, where the issue sets delta = 0."""
    D = c["D"] if D is None else D
    ref = reference64(c, pv)
    t = P_BITS[pv]
    smax = float(scores(c).abs().max())
    s = row_lsb(c)
    delta = (BIAS + smax) * 2.0 ** -24 * s
    if pv == "fp8":
        delta = delta + 2.0 ** -24 * (smax * s + FP8_OFFSET)
    if delta_zero:
        delta = torch.zeros_like(delta)
    rel = 2 * 2.0 ** -t + (torch.exp2(2 * delta) - 1) + 2.0 ** -18
    if pv == "fp16":
        sub = 2.0 ** -25 * ref["sumabsv"]
    elif pv == "bf16":
        sub = torch.zeros_like(ref["sumabsv"])
    else:
        sub = 2.0 ** -10 * 2.0 ** -(FP8_OFFSET - 3.0) * ref["sumabsv"]
    o_b = rel.unsqueeze(-1) * ref["wabsv"] + sub + 2 * out_ulp(ref["o"], pv, c.get("out_dtype"))
    l_b = delta + K_LOG2E * c["N"] * 2.0 ** -24 + 2 * _ulp(ref["lse2"], 23, -126)
    if D == 64 and pv == "fp16":
        l_b = l_b + math.log2(1 + 2.0 ** -11)
    return o_b, l_b


def ratios(c, pv, o, lse2):
    """largest |o - o64| / bound and |lse2 - lse2_64| / bound over ALL elements (no percentile); non-finite -> inf"""
    ref = reference64(c, pv)
    o_b, l_b = bound(c, pv)
    o, lse2 = o.double(), lse2.double()
    if not (torch.isfinite(o).all() and torch.isfinite(lse2).all()):
        return float("inf"), float("inf")
    return float(((o - ref["o"]).abs() / o_b).max()), float(((lse2 - ref["lse2"]).abs() / l_b).max())


# ---------------------------------------------------------------------------------------------------------------------
# the oracle on a case, and a float64 restatement of the kernel's loop that can make one deliberate mistake
# ---------------------------------------------------------------------------------------------------------------------

def v_of(c, pv):
    return {"fp16": c["v_f16"], "bf16": c["v_bf16"], "fp8": c["v_f8t"]}[pv]


def oracle(c, pv):
    """oracle.sage_oracle.attn_tile_loop, "hip" flavour, on the case -> (o in the output dtype, lse2 fp32)"""
    key, cache = ("oracle", pv), c.setdefault("_cache", {})
    if key not in cache:
        cache[key] = O.attn_tile_loop(c["q8"], c["k8"], v_of(c, pv), c["q_scale_rows"], c["k_scale_cols"],
                                  logit_mult=c["logit_mult"], is_causal=c["causal"], pv="fp8" if pv == "fp8" else "fp16",
                                  v_scale=c["v_scale"] if pv == "fp8" else None, out_dtype=OUT_DTYPE[pv], flavor="hip")
    return cache[key]


MISTAKES = ("swap_key_groups", "tile3_scales_of_tile2", "q_group_xor_1", "drop_last_key", "admit_key_N", "wrap_2_21",
            "clamp_p_2_5")


def restate64(c, pv, mistake=None):
    """The kernel's loop in float64 with NO rounding: 64-key tiles, a running maximum that is raised only when some row of
    the 32-row wave sees its tile maximum exceed m_run + kLazyThr (the wave-wide ballot), p = 2^(t - m_run).  Without a
    mistake it equals reference64 to float64 accuracy; ``mistake`` makes exactly one of MISTAKES."""
    M, N, gran = c["M"], c["N"], c["gran"]
    S = scores(c)
    q_rows, k_cols = c["q_scale_rows"], c["k_scale_cols"]
    V = v64(c, pv)
    ok = allowed(c).expand(1, HQ, M, N).clone()
    if mistake == "swap_key_groups":      # key groups 0/1 and 2/3 of every tile take each other's scale
        n = torch.arange(N)
        partner = torch.where(((n % 8) // 2) % 2 == 0, n + 2, n - 2).clamp(max=N - 1)
        k_cols = k_cols[:, :, partner]
    elif mistake == "tile3_scales_of_tile2":
        k_cols = k_cols.clone()
        k_cols[:, :, 192:256] = c["k_scale_cols"][:, :, 128:192]
    elif mistake == "q_group_xor_1":
        gid, ng = _gid_q(M, gran)
        q_rows = c["q_scale"][:, :, (gid ^ 1).clamp(max=ng - 1)]
    elif mistake == "drop_last_key":
        ok[..., N - 1] = False
    elif mistake == "admit_key_N":        # the zero padding after the last key: S = 0, V = 0, seen by every row
        S = torch.cat([S, torch.zeros(1, HQ, M, 1, dtype=S.dtype)], dim=-1)
        k_cols = torch.cat([k_cols, k_cols[:, :, -1:]], dim=-1)
        V = torch.cat([V, torch.zeros(1, HQ, 1, V.shape[-1], dtype=V.dtype)], dim=2)
        ok = torch.cat([ok, torch.ones(1, HQ, M, 1, dtype=torch.bool)], dim=-1)
    elif mistake == "wrap_2_21":          # a 22-bit accumulator: +2^21 becomes -2^21
        S = torch.remainder(S + 2.0 ** 21, 2.0 ** 22) - 2.0 ** 21
    t_all = (S * scale_matrix(c, q_rows, k_cols)).masked_fill(~ok, float("-inf"))
    thr = LAZY_THR[pv]
    NEG = float("-inf")
    m_run = torch.full((1, HQ, M), NEG, dtype=torch.float64)
    l = torch.zeros(1, HQ, M, dtype=torch.float64)
    acc = torch.zeros(1, HQ, M, V.shape[-1], dtype=torch.float64)
    wave = torch.arange(M) // 32
    nw = int(wave.max()) + 1
    for n0 in range(0, t_all.shape[-1], 64):
        t = t_all[..., n0:n0 + 64]
        mx = t.amax(-1)
        need = (mx > m_run + thr) | (torch.isinf(m_run) & ~torch.isinf(mx))
        wave_need = torch.stack([need[..., wave == w].any(-1) for w in range(nw)], dim=-1)
        do = wave_need[..., wave]
        m_new = torch.where(do, torch.maximum(m_run, mx), m_run)
        alpha = torch.where(torch.isinf(m_new), torch.ones_like(m_new),
                            torch.exp2(torch.where(torch.isinf(m_run), torch.full_like(m_run, NEG), m_run - m_new)))
        safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        p = torch.exp2(t - safe.unsqueeze(-1))
        if mistake == "clamp_p_2_5":
            p = p.clamp(max=32.0)
        l = l * alpha + p.sum(-1)
        acc = acc * alpha.unsqueeze(-1) + p @ V[:, :, n0:n0 + 64]
        m_run = m_new
    return acc / l.unsqueeze(-1), m_run + torch.log2(l)


# ---------------------------------------------------------------------------------------------------------------------
# which cases each family spans (shared by the CPU soundness test and the GPU test)
# ---------------------------------------------------------------------------------------------------------------------

FAMILIES = ("scale_ladder", "ramp", "extreme_s", "one_hot", "coarse_lsb", "big_v")


def family_cases(family, D, pv, grans=GRANS):
    """Yield (label, case) for one family at one head_dim and PV type.

    scale_ladder, ramp: the families that depend on the loop shape.  scale_ladder spans every N of LOOP_NS x causal x
      granularity.  ramp spans the five steps of its PV type (thr = 6 or 3) x causal x granularity; the ascending staircase
      at every N of LOOP_NS, the descending and sawtooth ones at N = 456 (their point is the order of the maxima, not the
      ring slot a tile lands in).
    extreme_s, one_hot, coarse_lsb, big_v: properties of one tile's arithmetic, N = 456 only (six full tiles and a ragged
      one), x causal x granularity."""
    g0 = grans[0]
    for causal in (False, True):
        if family in ("scale_ladder", "coarse_lsb", "big_v"):  # the scales, hence the logits, depend on the granularity
            for gran in grans:
                tag = f"{'causal' if causal else 'full'}-{gran}"
                if family == "scale_ladder":
                    for N in LOOP_NS:
                        yield f"N{N}-{tag}", scale_ladder(D, N, causal, gran)
                elif family == "coarse_lsb":
                    for e in (-6, -5, -4):
                        yield f"lsb2^{e}-{tag}", coarse_lsb(D, N_ONE, causal, gran, e)
                else:
                    yield tag, big_v(D, N_ONE, causal, gran)
            continue
        base = []  # uniform scales: one set of logits, laid out for each granularity
        if family == "ramp":
            for step in ramp_steps(pv):
                for shape in RAMP_SHAPES:
                    for N in (LOOP_NS if shape == "ascending" else (N_ONE,)):
                        base.append((f"{shape}-step{step}-N{N}", ramp(D, N, causal, g0, step, shape)))
        elif family == "extreme_s":
            for variant in ("corner", "zero"):
                base.append((variant, extreme_s(D, N_ONE, causal, g0, variant)))
        elif family == "one_hot":
            for where in ONE_HOT_KEYS:
                base.append((where, one_hot(D, N_ONE, causal, g0, where)))
                base.append((f"{where}-subnormal", one_hot(D, N_ONE, causal, g0, where, subnormal=True)))
        else:
            raise ValueError(family)
        for label, c in base:
            for gran in grans:
                yield f"{label}-{'causal' if causal else 'full'}-{gran}", (c if gran == g0 else regran(c, gran))


def uniform_case(v, causal, M):
    """The case a degenerate operator call reduces to: all logits equal (S = 0), so every row weighs its keys uniformly.
    ``v`` is the fp16 or bf16 V [1,1,N,D] the operator was given; the e4m3 triple is the operator's own quantizer
    (oracle.per_channel_fp8 without smoothing, bit-exact against the HIP quantizer in tests/test_gpu_parity.py).  The
    output dtype follows ``v``."""
    N, D = v.shape[2], v.shape[3]
    v8t, vsc, _ = O.per_channel_fp8(v, "HND", smooth_v=False)
    return dict(q8=torch.zeros(B, HQ, M, D, dtype=torch.int8), k8=torch.zeros(B, HK, N, D, dtype=torch.int8),
                q_scale_rows=torch.ones(B, HQ, M), k_scale_cols=torch.ones(B, HK, N), logit_mult=1.0, causal=causal,
                M=M, N=N, D=D, family="degenerate", v_f16=v, v_bf16=v, v_f8t=v8t, v_scale=vsc, out_dtype=v.dtype)
