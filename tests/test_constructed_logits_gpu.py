"""The attention kernels on CONSTRUCTED int8 operands and scales (tests/constructed_cases.py), against an fp64 softmax of
exactly those operands and a per-element bound derived from the roundings the kernel admits (constructed_cases.bound;
tests/test_constructed_cases.py proves on the CPU that the bound is sound and that it has teeth).  No quantizer noise, no
fitted number, no percentile: every element of o and lse2 is held to ratio <= 1.

Axes (constructed_cases.family_cases):
  scale_ladder, ramp -- they depend on the loop shape -- span N in {320, 384, 456, 512} (n_fast 4..7: four-slot ring exact,
    +1, +2, +3; two-slot ring even and odd; ragged last tile at 456) x causal x granularity x head_dim x PV x nwaves; the
    descending and sawtooth ramps run at N = 456 only (what they vary is the order of the tile maxima).
  extreme_s, one_hot, coarse_lsb, big_v are properties of one tile's arithmetic: N = 456, every other axis in full.
per_block goes in with logit_mult_is_one for FP16/BF16 PV (q_scale carries the 2^-3 of logit_mult); the FP8 shim has no
such argument, there every granularity takes logit_mult = sm_scale * log2(e) = 2^-3 exactly (constructed_cases.SM_SCALE)."""
import ctypes
import math

import pytest
import torch

import constructed_cases as C
from conftest import LSE2_TOL_FP32_P, LSE2_TOL_TWO_ROUNDED_P
from constructed_gpu_util import _Dev, _desc, _pinned

pytestmark = pytest.mark.gpu

_RECORD = {}


@pytest.fixture(scope="module")
def sa():
    assert torch.cuda.is_available()
    import sageattention_amd
    return sageattention_amd


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    if _RECORD:
        print("\nconstructed logits: largest |err| / bound over all elements   [o, lse2]")
        for (what, fam, pv, D), (ro, rl) in sorted(_RECORD.items()):
            print(f"  {what:8s} {fam:13s} {pv:5s} D={D:<4d} {ro:6.3f} {rl:6.3f}")


def _record(what, fam, pv, D, ro, rl):
    a, b = _RECORD.get((what, fam, pv, D), (0.0, 0.0))
    _RECORD[(what, fam, pv, D)] = (max(a, ro), max(b, rl))


def _second_check(c, pv, o, lse2):
    """scale_ladder and ramp have row LSBs <= 2^-12, the regime of the existing kernel tests: the oracle's "hip" flavour under
    the tolerances of test_gpu_parity.test_attention_kernel_vs_reference_and_oracle (2 output ulps with the 0.25 floor,
    conftest.LSE2_TOL_*) -> the two error figures in units of those tolerances"""
    oo, ol = C.oracle(c, pv)
    ulp = 2.0 ** -10 if C.OUT_DTYPE[pv] == torch.float16 else 2.0 ** -7
    ro = float(((o.float() - oo.float()).abs() / (2 * ulp * oo.float().abs().clamp(min=0.25))).max())
    tol = LSE2_TOL_TWO_ROUNDED_P if c["D"] <= 64 else LSE2_TOL_FP32_P
    return ro, float((lse2 - ol).abs().max()) / tol


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", C.FAMILIES)
def test_dense_kernels_within_the_derived_bound(sa, family, pv, D):
    bad = []
    for label, c in C.family_cases(family, D, pv):
        dev = _Dev(sa, c, pv)
        for nw in (4, 8):
            with _pinned(nw):
                o, lse2 = dev.dense(sa)
            o, lse2 = o.cpu(), lse2.cpu()
            ro, rl = C.ratios(c, pv, o, lse2)
            _record("dense", family, pv, D, ro, rl)
            if not (ro <= 1.0 and rl <= 1.0):
                bad.append((label, nw, "bound", ro, rl))
            if family in ("scale_ladder", "ramp") and pv != "fp8":
                assert float(C.row_lsb(c).max()) <= 2.0 ** -12
                so, sl = _second_check(c, pv, o, lse2)
                _record("vs-hip", family, pv, D, so, sl)  # in units of the existing tolerances, strict '<' as there
                if not (so <= 1.0 and sl < 1.0):
                    bad.append((label, nw, "oracle", so, sl))
    assert not bad, bad[:20]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", C.PVS)
@pytest.mark.parametrize("family", ["scale_ladder", "ramp"])
def test_block_sparse_all_ones_is_bit_identical_to_dense(sa, family, pv, D):
    """an all-ones map, compacted into a plan beforehand, through the block-sparse entry points: the same loop body, o and
    the raw lse2 bit-identical to the dense kernel in the sparse kernel's 4-wave geometry (README, block-sparse section)"""
    from sageattention_amd import _lib as L
    for label, c in C.family_cases(family, D, pv):
        if c["causal"] or c["N"] != C.N_ONE:
            continue  # the block-sparse kernels are non-causal
        M, N = c["M"], c["N"]
        dev = _Dev(sa, c, pv)
        with _pinned(4):
            o_d, l_d = dev.dense(sa)
        ones = torch.ones(1, 1, (M + 127) // 128, (N + 63) // 64, dtype=torch.bool, device="cuda")
        lists = sa.block_sparse_plan(ones, M, N, B=C.B, Hq=C.HQ).lists
        o, lse = dev.out(), torch.full((C.B, C.HQ, M), float("nan"), device="cuda")
        warpq = 128 if c["gran"] == "per_block" else 32
        tail = (None, lse.data_ptr(), C.B, C.HQ, C.HK, M, N, D, 0, dev.code, 128, warpq, c["sm_scale"], 0,
                lists.data_ptr(), lists.numel() * 4, L.stream_ptr(o.device))
        mid = (_desc(L, o), L.dtype_code(o.dtype), dev.qs.data_ptr(), dev.ks.data_ptr())
        head = (_desc(L, dev.q8), _desc(L, dev.k8), _desc(L, dev.v))
        if pv == "fp8":
            L.check(L.lib().sage_attn_qk_int8_pv_f8_blocksparse(*head, *mid, dev.v_scale.data_ptr(), *tail), "f8 blocksparse")
        else:
            L.check(L.lib().sage_attn_qk_int8_pv_f16_blocksparse(*head, L.dtype_code(dev.v.dtype), *mid, *tail), "f16 blocksparse")
        torch.cuda.synchronize()
        if pv != "fp8" and c["gran"] == "per_block":
            # the dense call above folded logit_mult into q_scale; run it unfolded too so both sides got the same arguments
            with _pinned(4):
                o_d = dev.out()
                l_d = sa._qattn._attn_f16(dev.q8, dev.k8, dev.v, o_d, dev.qs, dev.ks, None, 1, False, dev.code, c["sm_scale"], 1)
                torch.cuda.synchronize()
        assert torch.equal(o, o_d) and torch.equal(lse, l_d), label
        ro, rl = C.ratios(c, pv, o.cpu(), lse.cpu())
        _record("sparse", family, pv, D, ro, rl)
        assert ro <= 1.0 and rl <= 1.0, (label, ro, rl)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pv", ["fp16", "bf16"])
@pytest.mark.parametrize("family", ["scale_ladder", "ramp"])
def test_attn_mask_entry_with_a_mask_that_masks_nothing(sa, family, pv, D):
    """the attn_mask entry sends every tile through the generic body: an all-true bool mask and an additive mask of zeros (in
    V's dtype) must stay inside the same fp64 bound -- the additive form rounds t = S*scale once more in fp32, which is
    2^-24 |t| and far inside delta.  No bit-identity with the dense kernel is claimed."""
    from sageattention_amd import _lib as L
    bad = []
    for label, c in C.family_cases(family, D, pv):
        if c["causal"] or c["N"] != C.N_ONE:
            continue  # attn_mask exists for non-causal calls only
        M, N = c["M"], c["N"]
        dev = _Dev(sa, c, pv)
        masks = [(1, torch.ones(C.B, C.HQ, M, N, dtype=torch.bool, device="cuda")),
                 (2 if pv == "fp16" else 3, torch.zeros(C.B, C.HQ, M, N, dtype=C.OUT_DTYPE[pv], device="cuda"))]
        warpq = 128 if c["gran"] == "per_block" else 32
        for kind, mask in masks:
            st = (ctypes.c_int64 * 4)(*mask.stride())
            for nw in (4, 8):
                o, lse = dev.out(), torch.full((C.B, C.HQ, M), float("nan"), device="cuda")
                with _pinned(nw):
                    L.check(L.lib().sage_attn_qk_int8_pv_f16_masked(
                        _desc(L, dev.q8), _desc(L, dev.k8), _desc(L, dev.v), L.dtype_code(dev.v.dtype), _desc(L, o),
                        L.dtype_code(o.dtype), dev.qs.data_ptr(), dev.ks.data_ptr(), mask.data_ptr(), kind, st, lse.data_ptr(),
                        C.B, C.HQ, C.HK, M, N, D, dev.code, 128, warpq, c["sm_scale"], 0, L.stream_ptr(o.device)), "masked")
                    torch.cuda.synchronize()
                ro, rl = C.ratios(c, pv, o.cpu(), lse.cpu())
                _record("mask", family, pv, D, ro, rl)
                if not (ro <= 1.0 and rl <= 1.0):
                    bad.append((label, kind, nw, ro, rl))
    assert not bad, bad[:20]


# ---- the fused Q quantizer and the operators on degenerate inputs -------------------------------------------------------

def _degenerate_inputs(dtype, D, causal):
    """Q with rows 32..63 and the whole second 128-row q-block zero, a constant K (one row repeated), random V.  Q and K hold
    multiples of 1/8 in [-4, 4]: the k mean (456 equal addends), K - mean = 0 and the LSE correction q.km are then EXACT in
    fp32 whatever the summation order, so the expected values need no allowance for them."""
    N = 456
    M = N if causal else 150
    g = torch.Generator().manual_seed(900 + D)
    q = (torch.randint(-32, 33, (1, 2, M, D), generator=g).float() / 8)
    q[:, :, 32:64] = 0
    q[:, :, 128:256] = 0
    k = (torch.randint(-32, 33, (1, 1, 1, D), generator=g).float() / 8).expand(1, 1, N, D).contiguous()
    v = torch.randn(1, 1, N, D, generator=g)
    return q.to(dtype), k.to(dtype), v.to(dtype)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_operators_on_zero_q_rows_and_constant_k(sa, monkeypatch, pv, dtype, D):
    """All logits of a row are equal (K minus its mean is zero), so o is the mean of V over the row's keys (causal: the prefix
    mean) within the bound with delta = 0 -- a common shift of a tile's exponent cannot move equal weights apart -- and
    lse = q.k / sqrt(d) + ln(keys).  LSE tolerance: the lse2 bound (delta = 0) times ln 2, plus four fp32 roundings of the
    finishing step lse2 / log2(e) + (q.km) * sm_scale (sm_scale itself, the product, the quotient, the sum), each at most
    2^-24 of the largest magnitude involved.  One-call and multi-call paths, and in the multi-call path the fused Q quantizer
    bit-identical to the stand-alone one."""
    op = sa.sageattn_qk_int8_pv_fp16_cuda if pv == "fp16" else sa.sageattn_qk_int8_pv_fp8_cuda
    kind = "fp8" if pv == "fp8" else ("fp16" if dtype == torch.float16 else "bf16")
    for causal in (False, True):
        q, k, v = _degenerate_inputs(dtype, D, causal)
        M, N = q.shape[2], k.shape[2]
        c = C.uniform_case(v, causal, M)
        ref = C.reference64(c, kind)
        o_b, l2_b = C.bound(c, kind, delta_zero=True)
        keys = (torch.arange(1, M + 1).clamp(max=N) if causal else torch.full((M,), N)).double()
        qk = (q.double() * k.double()[:, :, :1]).sum(-1) * D ** -0.5
        lse64 = qk + torch.log(keys).view(1, 1, M)
        l_b = l2_b * math.log(2) + 4 * 2.0 ** -24 * torch.maximum(qk.abs(), lse64.abs()).clamp(min=math.log(N))
        assert (ref["lse2"] - torch.log2(keys).view(1, 1, M)).abs().max() < 1e-12  # the reduced case IS the uniform one
        qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
        for gran in ("per_warp", "per_thread"):
            res = {}
            for route, one_call, fuse in (("one-call", True, True), ("fused-q", False, True), ("separate-q", False, False)):
                monkeypatch.setattr(sa.core, "ONE_CALL", one_call)
                monkeypatch.setattr(sa.core, "FUSE_Q_QUANT", fuse)
                o, lse = op(qc, kc, vc, is_causal=causal, qk_quant_gran=gran, return_lse=True)
                torch.cuda.synchronize()
                res[route] = (o, lse)
                o, lse = o.cpu(), lse.cpu()
                assert o.dtype == dtype and torch.isfinite(o).all() and torch.isfinite(lse).all(), (route, gran, causal)
                ro = float(((o.double() - ref["o"]).abs() / o_b).max())
                rl = float(((lse.double() - lse64).abs() / l_b).max())
                _record("operator", "degenerate", kind, D, ro, rl)
                assert ro <= 1.0 and rl <= 1.0, (route, gran, causal, ro, rl)
            assert torch.equal(res["fused-q"][0], res["separate-q"][0]) and torch.equal(res["fused-q"][1], res["separate-q"][1])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_fused_q_reproduces_a_chosen_q8_bit_for_bit(sa, dtype, D):
    """per_warp: Q = q8 * 2^e per 32-row group, every group holding a +-127.  Then amax / 127 = 2^e and 127 / amax = 2^-e
    exactly, the quantizer must give back the chosen q8 and scales, and the fused-Q kernel must equal the int8 entry point fed
    that q8: o and the finished LSE bit for bit."""
    from sageattention_amd import core
    for causal in (False, True):
        c = C.scale_ladder(D, 456, causal, "per_warp")
        M, N = c["M"], c["N"]
        q8 = c["q8"].clone()
        q8[:, :, 0::32, 0] = torch.tensor([127, -127]).repeat((M + 31) // 32 // 2 + 1)[:(M + 31) // 32].to(torch.int8)
        e = torch.tensor([3, -2, 0, 5, -6, 1, -4, 2]).repeat(M // 256 + 1)  # per 32-row group, fp16-exact products
        ng = c["q_scale"].shape[-1]
        scale = torch.pow(2.0, e[:ng].float()).view(1, 1, ng) * torch.tensor([1.0, 0.5]).view(1, 2, 1)
        q = (q8.float() * C.O.expand_q_scale(scale, M, "per_warp").unsqueeze(-1)).to(dtype)
        assert torch.equal(q.float(), q8.float() * C.O.expand_q_scale(scale, M, "per_warp").unsqueeze(-1))  # exact
        # K = a constant row + noise in +- pairs, all multiples of 1/8: its mean is that row exactly, and q.km (multiples of
        # 2^(e-3), below 2^(e+16)) is exact in fp32 in ANY summation order -- the fused prologue and the stand-alone quantizer
        # sum it differently (test_gpu_parity.test_fused_q_quantizer_is_bit_identical), here that cannot show
        g = torch.Generator().manual_seed(950 + D)
        k0 = torch.randint(-32, 33, (1, 1, 1, D), generator=g).float() / 8
        noise = torch.randint(-16, 17, (1, 1, N // 2, D), generator=g).float() / 8
        k = (k0 + torch.stack([noise, -noise], dim=3).view(1, 1, N, D)).to(dtype)
        v = torch.randn(1, 1, N, D, generator=g).to(dtype)
        qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
        sm = D ** -0.5
        k8, ks, km = core._prep_k(kc, "HND", "per_warp", True)
        assert torch.equal(km.cpu().float().view(-1), k0.view(-1))
        q8x, qsx, corr = core._quant_q(qc, km, "HND", "per_warp", sm, 32, True, 2, 1)
        assert torch.equal(q8x.cpu(), q8)
        assert torch.equal(qsx.cpu()[..., :(M + 31) // 32], scale[..., :(M + 31) // 32])
        o_f, lse_f = core._fused_attn(qc, (k8, ks, km, vc, None, None), "HND", causal, ("per_warp", 32), sm, True)
        o_s = torch.empty_like(qc)
        lse2 = sa._qattn._attn_f16(q8.cuda(), k8, vc, o_s, qsx, ks, None, 1, int(causal), 2, sm, 1)
        lse_s = core._finish_lse(lse2, corr, sm)
        torch.cuda.synchronize()
        assert torch.equal(o_f, o_s) and torch.equal(lse_f, lse_s), causal
