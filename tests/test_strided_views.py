"""Every entry point on strided views inside poisoned memory (tests/view_cases.py).

The kernels receive the caller's strides (a slice of a packed QKV projection, a prefix of a KV cache, a head or batch
slice, an expanded head), and a contiguous tensor ties those strides to the sizes, so a kernel that derives one stride from
another, reads a row past N, or writes next to its output passes every test that only uses contiguous tensors.  Each case
here runs one call with one argument (or all of them) given as a view whose surroundings are poison and runs it again on
fresh contiguous copies, then asserts
  (a) the same BITS as the contiguous call for every output (no tolerance: strides select bytes, not arithmetic),
  (b) agreement with the CPU oracle computed from the logical values, with the assertion of the named existing test,
  (c) finite outputs (no poison leaked),
  (d) every byte of an output's parent outside the view still holds the sentinel, every element inside was written, and
      the parents of the inputs are unchanged bit for bit.
No case needed the fall-back from (a) to (b)."""
import ctypes
import hashlib

import pytest
import torch

import view_cases as V
from conftest import LSE2_TOL_FP32_P, LSE2_TOL_ROUNDED_P

pytestmark = pytest.mark.gpu

DEV = "cuda"
LOG2E = 1.4426950408889634
F16, BF16, I8, F8, F32 = torch.float16, torch.bfloat16, torch.int8, torch.float8_e4m3fn, torch.float32


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from sageattention_amd import _lib
    _lib.lib()
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(V.raw_bytes(a.contiguous()), V.raw_bytes(b.contiguous()))


class Dense:
    """An array the C ABI takes as a plain contiguous pointer (scales, km, lse, ...), inside sentinel guards."""
    PAD = 64

    def __init__(self, shape, dtype=F32, full=True):
        self.full = full  # every element must be written
        n = 1
        for s in shape:
            n *= s
        self.parent = V.sentinel((n + 2 * self.PAD,), dtype).to(DEV)
        self.t = self.parent[self.PAD:self.PAD + n].view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def result(self, name):
        raw = V.raw_bytes(self.parent).cpu()
        g = self.PAD * self.parent.dtype.itemsize
        assert (raw[:g] == 0xFF).all() and (raw[-g:] == 0xFF).all(), f"{name}: written outside its exact length"
        if self.full:
            assert not (raw[g:-g].view(-1, self.parent.dtype.itemsize) == 0xFF).all(dim=1).any(), f"{name}: element not written"
        return self.t.cpu().clone()


class Case:
    """The tensors of one call: every input named in ``kinds`` a poisoned view, every other one a fresh contiguous tensor;
    every output a view of a sentinel-filled parent (``contiguous`` = a dense one)."""

    def __init__(self, inputs, outputs, kinds, seed):
        self.ins, self.outs, self.t = {}, {}, {}
        for i, (name, val) in enumerate(inputs.items()):
            c = V.make_input(kinds.get(name, "contiguous"), values=val, seed=seed + i).to(DEV)
            self.ins[name], self.t[name] = c, c.view
        for i, (name, (shape, dtype)) in enumerate(outputs.items()):
            c = V.make_output(kinds.get(name, "contiguous"), shape, dtype, seed=seed + i).to(DEV)
            self.outs[name], self.t[name] = c, c.view
        self.logical = {n: c.logical for n, c in self.ins.items()}

    def finish(self):
        """Assertion (d); -> the outputs as contiguous CPU tensors."""
        torch.cuda.synchronize()
        for n, c in self.ins.items():
            assert c.parent_unchanged(), f"input {n} ({c.kind}) was modified"
        for n, c in self.outs.items():
            assert c.outside_untouched(), f"output {n} ({c.kind}): bytes outside the view were written"
            if c.view.dtype != I8:
                assert c.all_written(), f"output {n} ({c.kind}): elements of the view were not written"
        return {n: c.view.contiguous().cpu() for n, c in self.outs.items()}


def run_both(call, inputs, outputs, kinds, seed=0):
    """``call(t) -> {name: Dense}`` on the views and on contiguous copies of their logical values; asserts (a) and (d).
    -> (results of the view call, logical inputs)"""
    res = []
    case = Case(inputs, outputs, kinds, seed)
    for c in (case, Case(case.logical, outputs, {}, seed)):
        dense = call(c.t)
        r = c.finish()
        r.update({n: d.result(n) for n, d in dense.items()})
        res.append(r)
    got, ref = res
    assert got.keys() == ref.keys()
    for n in ref:
        assert _same_bits(got[n], ref[n]), f"{n}: differs from the contiguous call in {int((V.raw_bytes(got[n]) != V.raw_bytes(ref[n])).sum())} bytes ({kinds})"
    return got, case.logical


def arg_cases(in_args, out_args, everything):
    """One case per (argument, kind) and one with every argument a view of a different kind."""
    out = [pytest.param({a: k}, id=f"{a}-{k}") for a in in_args for k in V.INPUT_KINDS]
    out += [pytest.param({a: k}, id=f"{a}-{k}") for a in out_args for k in V.OUTPUT_KINDS]
    return out + [pytest.param(everything, id="all-" + "-".join(everything.values()))]


def d4(L, t):
    return L.SageTensor(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def code(L, dt):
    return L.SAGE_F16 if dt == F16 else L.SAGE_BF16


_memo = {}


def memo(tag, tensors, fn):
    """The oracle once per distinct set of logical inputs (the per-argument cases of one configuration share them)."""
    h = hashlib.sha1(repr(tag).encode())
    for t in tensors:
        h.update(V.raw_bytes(t.contiguous()).numpy().tobytes())
    key = h.hexdigest()
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def ws_for(nbytes):
    return torch.empty(max(1, nbytes), dtype=torch.uint8, device=DEV)


# ---- K mean ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", arg_cases(["k"], [], {"k": "kv_cache"})[:-1])
@pytest.mark.parametrize("cfg", [(2, 3, 333, 64, F16), (2, 2, 1027, 128, BF16)], ids=str)
def test_k_mean(L, cfg, kinds):
    """sage_k_mean; (b) as test_gpu_parity.test_k_mean_vs_reference: within one ulp of the storage dtype."""
    from oracle import sage_oracle as O
    B, H, N, D, dt = cfg
    k = V.random_values((B, H, N, D), dt, 1, channel_bias=2.0)

    def call(t):
        km = Dense((B, H, D), dt)
        ws = ws_for(L.lib().sage_k_mean_workspace_bytes(B, H, N, D))
        assert L.lib().sage_k_mean(d4(L, t["k"]), code(L, dt), B, H, N, D, km.ptr(), ws.data_ptr(), _stream()) == 0
        return {"km": km}
    got, lg = run_both(call, {"k": k}, {}, kinds)
    ref = O.k_mean(lg["k"]).squeeze(2).float()
    ulp = 2.0 ** -10 if dt == F16 else 2.0 ** -7
    assert torch.isfinite(got["km"]).all()
    assert ((got["km"].float() - ref).abs() <= ulp * ref.abs().clamp(min=2.0 ** -14)).all()


# ---- INT8 quantizer -------------------------------------------------------------------------------------------------------
QUANT_CFGS = [
    # (name, is_key, gran, blk, warp, rounding, with lse_dot, dtype, (B, H, N, D))
    ("q_block_triton", 0, 1, 128, 128, 0, False, F16, (2, 2, 200, 64)),
    ("q_warp32_cuda_dot", 0, 2, 128, 32, 1, True, BF16, (2, 4, 333, 128)),
    ("q_warp16_cuda", 0, 2, 128, 16, 1, False, F16, (2, 2, 77, 128)),
    ("q_thread_triton_dot", 0, 3, 128, 32, 0, True, F16, (2, 4, 77, 64)),
    ("k_block_triton_mean", 1, 1, 64, 64, 0, False, F16, (2, 2, 77, 128)),
    ("k_block_cuda_mean", 1, 1, 64, 64, 1, False, F16, (2, 3, 333, 64)),
    ("k_thread_triton_mean", 1, 3, 64, 64, 0, False, BF16, (2, 2, 200, 128)),
]


def _oracle_quant(O, x, km, is_key, gran, warp, rounding, sm_scale):
    """-> (int8, scales) of the role's half of the reference pairing."""
    if gran == 1:
        r = O.per_block_int8(x, x, km, sm_scale=sm_scale, rounding="cuda" if rounding else "triton")
    elif gran == 2:
        r = O.per_warp_int8(x, x, km, WARPQ=warp)
    else:
        r = O.per_thread_int8(x, x, km)
    return (r[2], r[3]) if is_key else (r[0], r[1])


@pytest.mark.parametrize("kinds", arg_cases(["x"], ["out"], {"x": "seq_slice", "out": "packed_nhd"}))
@pytest.mark.parametrize("cfg", QUANT_CFGS, ids=lambda c: c[0])
def test_quant_qk_int8(L, cfg, kinds):
    """sage_quant_qk_int8 in the Q and K roles; (b) bit-exact against the oracle's quantizers, as
    test_gpu_parity.test_quant_per_{block,thread}_bit_exact_vs_reference / test_quant_per_warp_bit_exact_vs_oracle.  The
    fused q.km dot enters the LSE as lse_dot * sm_scale: the LSE bound of test_edge_shapes_vs_oracle (2e-3)."""
    from oracle import sage_oracle as O
    name, is_key, gran, blk, warp, rounding, dot, dt, (B, H, N, D) = cfg
    x = V.random_values((B, H, N, D), dt, 2, channel_bias=1.5 if is_key else 0.0)
    sm = D ** -0.5
    mult = sm * 1.44269504 if (gran == 1 and not is_key) else 1.0
    G = (N + blk - 1) // blk * (1 if gran == 1 else (blk // warp) * (1 if gran == 2 else (4 if is_key else 8)))
    group = 2 if dot else 1
    vec = V.random_values((B, H // group, 1, D), dt, 3).squeeze(2).contiguous() if dot else None

    def call(t):
        lg = t["x"].contiguous().cpu()
        km = O.k_mean(lg).squeeze(2).contiguous().to(DEV) if is_key else None
        scale, ld = Dense((B, H, G)), Dense((B, H, N)) if dot else None
        vec_d = vec.to(DEV) if dot else None
        st = L.lib().sage_quant_qk_int8(d4(L, t["x"]), code(L, dt), B, H, N, D, L.ptr(km), d4(L, t["out"]), scale.ptr(), gran,
                                        is_key, blk, warp, float(mult), rounding, L.ptr(vec_d), group, ld.ptr() if dot else None,
                                        _stream())
        assert st == 0, st
        return {"scale": scale, **({"lse_dot": ld} if dot else {})}
    got, lg = run_both(call, {"x": x}, {"out": ((B, H, N, D), I8)}, kinds)
    km = O.k_mean(lg["x"]) if is_key else None
    r8, rs = memo(cfg[:7], [lg["x"]], lambda: _oracle_quant(O, lg["x"], km, is_key, gran, warp, rounding, sm))
    assert torch.isfinite(got["scale"]).all()
    assert torch.equal(got["scale"], rs) and torch.equal(got["out"], r8), int((got["out"] != r8).sum())
    if dot:
        want = O.lse_correction(lg["x"], vec.unsqueeze(2))
        assert torch.isfinite(got["lse_dot"]).all() and ((got["lse_dot"] - want) * sm).abs().max() < 2e-3


# ---- V smoothing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", arg_cases(["v"], ["out"], {"v": "kv_cache", "out": "row_padded"}))
@pytest.mark.parametrize("cfg", [(2, 3, 333, 128, BF16), (2, 2, 77, 64, F16)], ids=str)
def test_sub_mean(L, cfg, kinds):
    """sage_sub_mean_f16; (b) bit-exact given the mean, as test_gpu_parity.test_sub_mean_bit_exact_vs_oracle."""
    from oracle import sage_oracle as O
    B, H, N, D, dt = cfg
    v = V.random_values((B, H, N, D), dt, 4, scale=2.0, channel_bias=3.0)

    def call(t):
        vm = O.sub_mean(t["v"].contiguous().cpu())[1].contiguous().to(DEV)
        assert L.lib().sage_sub_mean_f16(d4(L, t["v"]), code(L, dt), B, H, N, D, vm.data_ptr(), d4(L, t["out"]), _stream()) == 0
        return {}
    got, lg = run_both(call, {"v": v}, {"out": ((B, H, N, D), F16)}, kinds)
    want, _ = O.sub_mean(lg["v"], vm=O.sub_mean(lg["v"])[1])
    assert torch.isfinite(got["out"]).all() and torch.equal(got["out"], want)


# ---- FP8 V quantizer ------------------------------------------------------------------------------------------------------
def _mfma_index(npad):
    from sageattention_amd.quant import fp8_token_order
    return (torch.arange(npad // 64).view(-1, 1) * 64 + fp8_token_order().view(1, -1)).reshape(-1)  # position -> token


def _check_fp8_image(got8, got_scale, got_mean, v, N, smooth):
    """The assertions of test_gpu_parity.test_v_fp8_quantizer_vs_oracle on an image [B,H,D,Npad] (uint8 view)."""
    from oracle import sage_oracle as O
    r8, rs, rm = O.per_channel_fp8(v, smooth_v=smooth)
    idx = _mfma_index(got8.shape[-1])
    got, want = got8.view(torch.uint8), r8.view(torch.uint8)[..., idx]
    valid = idx < N
    assert (got[..., ~valid] == 0).all(), "token columns in [N, Npad) must be zero"
    got, want = got[..., valid], want[..., valid]
    assert torch.isfinite(got_scale).all()
    if smooth:
        assert torch.allclose(got_mean, rm, rtol=1e-5, atol=1e-6) and torch.allclose(got_scale, rs, rtol=1e-5, atol=0)
    else:
        assert torch.equal(got_scale, rs) and torch.equal(got, want), int((got != want).sum())
    assert (got != want).float().mean() < 5e-3 and (got.int() - want.int()).abs().max() <= 1


@pytest.mark.parametrize("kinds", arg_cases(["v"], ["v_fp8"], {"v": "packed_nhd", "v_fp8": "head_batch_slice"}))
@pytest.mark.parametrize("cfg", [(2, 3, 333, 128, BF16, False), (2, 2, 77, 64, F16, True), (2, 2, 200, 64, F16, False)], ids=str)
def test_quant_v_fp8(L, cfg, kinds):
    """sage_quant_v_fp8 with and without the channel mean; the image is an output view: its zero columns are asserted."""
    B, H, N, D, dt, smooth = cfg
    npad = (N + 63) // 64 * 64
    v = V.random_values((B, H, N, D), dt, 5, scale=1.5, channel_bias=1.0 if smooth else 0.0)

    def call(t):
        vs, vm = Dense((B, H, D)), Dense((B, H, D)) if smooth else None
        ws = ws_for(L.lib().sage_quant_v_fp8_workspace_bytes(B, H, N, D))
        st = L.lib().sage_quant_v_fp8(d4(L, t["v"]), code(L, dt), B, H, N, D, d4(L, t["v_fp8"]), vs.ptr(),
                                      vm.ptr() if smooth else None, 448.0, ws.data_ptr(), _stream())
        assert st == 0, st
        return {"v_scale": vs, **({"v_mean": vm} if smooth else {})}
    got, lg = run_both(call, {"v": v}, {"v_fp8": ((B, H, D, npad), F8)}, kinds)
    _check_fp8_image(got["v_fp8"], got["v_scale"], got.get("v_mean"), lg["v"], N, smooth)


# ---- K smoothing + quantization, and the whole K/V pre-pass ---------------------------------------------------------------
def _check_k_smooth(O, got, k, gran, rounding, dt):
    """km within one ulp of the oracle's mean (test_k_mean_vs_reference); int8 and scales bit-exact GIVEN that mean, as
    test_k_smooth_quant_is_bit_identical_to_mean_plus_quantizer pins them to the quantizer the oracle restates."""
    ref = O.k_mean(k).squeeze(2).float()
    ulp = 2.0 ** -10 if dt == F16 else 2.0 ** -7
    assert torch.isfinite(got["km"]).all() and torch.isfinite(got["scale"]).all()
    assert ((got["km"].float() - ref).abs() <= ulp * ref.abs().clamp(min=2.0 ** -14)).all()
    r8, rs = _oracle_quant(O, k, got["km"], 1, gran, 64, rounding, 1.0)
    assert torch.equal(got["scale"], rs) and torch.equal(got["k8"], r8), int((got["k8"] != r8).sum())


@pytest.mark.parametrize("kinds", arg_cases(["k"], ["k8"], {"k": "packed_hnd", "k8": "seq_slice"}))
@pytest.mark.parametrize("cfg", [(2, 3, 333, 64, F16, 3, 0), (2, 2, 1027, 128, BF16, 1, 1)], ids=str)
def test_k_smooth_quant(L, cfg, kinds):
    from oracle import sage_oracle as O
    B, H, N, D, dt, gran, rounding = cfg
    k = V.random_values((B, H, N, D), dt, 6, channel_bias=2.0)
    G = (N + 63) // 64 * (4 if gran == 3 else 1)

    def call(t):
        scale, km = Dense((B, H, G)), Dense((B, H, D), dt)
        ws = ws_for(L.lib().sage_k_mean_workspace_bytes(B, H, N, D))
        st = L.lib().sage_k_smooth_quant(d4(L, t["k"]), code(L, dt), B, H, N, D, d4(L, t["k8"]), scale.ptr(), km.ptr(), gran,
                                         rounding, ws.data_ptr(), _stream())
        assert st == 0, st
        return {"scale": scale, "km": km}
    got, lg = run_both(call, {"k": k}, {"k8": ((B, H, N, D), I8)}, kinds)
    _check_k_smooth(O, got, lg["k"], gran, rounding, dt)


@pytest.mark.parametrize("kinds", arg_cases(["k", "v"], ["k8", "v_fp8"],
                                            {"k": "kv_cache", "v": "kv_cache", "k8": "packed_nhd", "v_fp8": "row_padded"}))
@pytest.mark.parametrize("cfg", [(2, 2, 333, 128, F16, 3, 0), (2, 3, 200, 64, BF16, 1, 1)], ids=str)
def test_kv_prepare_fp8(L, cfg, kinds):
    from oracle import sage_oracle as O
    B, H, N, D, dt, gran, rounding = cfg
    npad = (N + 63) // 64 * 64
    k = V.random_values((B, H, N, D), dt, 7, channel_bias=2.0)
    v = V.random_values((B, H, N, D), dt, 8, scale=1.5)
    G = (N + 63) // 64 * (4 if gran == 3 else 1)

    def call(t):
        scale, km, vs = Dense((B, H, G)), Dense((B, H, D), dt), Dense((B, H, D))
        ws = ws_for(L.lib().sage_kv_prepare_fp8_workspace_bytes(B, H, N, D))
        st = L.lib().sage_kv_prepare_fp8(d4(L, t["k"]), d4(L, t["v"]), code(L, dt), B, H, N, D, d4(L, t["k8"]), scale.ptr(),
                                         km.ptr(), gran, rounding, d4(L, t["v_fp8"]), vs.ptr(), 448.0, ws.data_ptr(), _stream())
        assert st == 0, st
        return {"scale": scale, "km": km, "v_scale": vs}
    got, lg = run_both(call, {"k": k, "v": v}, {"k8": ((B, H, N, D), I8), "v_fp8": ((B, H, D, npad), F8)}, kinds)
    _check_k_smooth(O, got, lg["k"], gran, rounding, dt)
    _check_fp8_image(got["v_fp8"], got["v_scale"], None, lg["v"], N, False)


# ---- attention ------------------------------------------------------------------------------------------------------------
def _operands(O, cfg, seed):
    """fp16 q, k, v of a configuration and their quantized forms from the oracle (per_thread pairing)."""
    B, Hq, Hk, M, N, D = cfg[:6]
    q = V.random_values((B, Hq, M, D), F16, seed)
    k = V.random_values((B, Hk, N, D), F16, seed + 1, channel_bias=1.5)
    v = V.random_values((B, Hk, N, D), F16, seed + 2)
    km = O.k_mean(k)
    q8, qs, k8, ks = O.per_thread_int8(q, k, km)
    r8, vsc, _ = O.per_channel_fp8(v, smooth_v=False)
    img = r8.view(torch.uint8)[..., _mfma_index(r8.shape[-1])].contiguous().view(F8)  # the kernel's token order
    return dict(q=q, k=k, v=v, km=km.squeeze(2).contiguous(), q8=q8, qs=qs, k8=k8, ks=ks, v_fp8=img, v_scale=vsc)


def _unpermute(img):
    npad = img.shape[-1]
    out = torch.empty_like(img.view(torch.uint8))
    out[..., _mfma_index(npad)] = img.view(torch.uint8)
    return out.view(F8)


def _attn_oracle(O, lg, ops, cfg, pv, q8=None, qs=None, mask=None):
    B, Hq, Hk, M, N, D, causal = cfg[:7]
    q8 = lg["q8"] if q8 is None else q8
    v = lg["v"] if pv == "fp16" else _unpermute(lg["v_fp8"])
    return O.attn_tile_loop(q8, lg["k8"], v, O.expand_q_scale(ops["qs"] if qs is None else qs, M, "per_thread"),
                            O.expand_k_scale(ops["ks"], N, "per_thread"), logit_mult=D ** -0.5 * LOG2E, is_causal=causal,
                            pv=pv, v_scale=ops["v_scale"] if pv == "fp8" else None, flavor="hip", attn_mask=mask)


def _check_attn(got, oo, ol, pv, lse_is_base2=True):
    """(b), (c) with the bounds of test_gpu_parity.test_edge_shapes_vs_oracle: 2e-3 (FP16 PV) / 0.06 (FP8 PV) on o, 2e-3 on
    the natural-log LSE."""
    assert torch.isfinite(got["o"]).all() and torch.isfinite(got["lse"]).all()
    assert (got["o"].float() - oo.float()).abs().max() < (2e-3 if pv == "fp16" else 0.06)
    lse = got["lse"] / LOG2E if lse_is_base2 else got["lse"]
    assert (lse - ol).abs().max() < 2e-3


ATTN_CFGS = [
    # (B, Hq, Hk, M, N, D, causal, nwaves)
    (2, 4, 2, 200, 333, 64, False, 8),
    (2, 2, 2, 333, 333, 128, True, 4),
]
ATTN_LONG = (1, 2, 1, 4200, 4133, 128, True, 8)   # several query blocks, GQA, every argument a view
ATTN_ALL = {"q8": "packed_nhd", "k8": "kv_cache", "v": "seq_slice", "o": "head_batch_slice"}
ATTN_CASES = [(c, k) for c in ATTN_CFGS for k in arg_cases(["q8", "k8", "v"], ["o"], ATTN_ALL)] + \
             [(ATTN_LONG, pytest.param(ATTN_ALL, id="all-long"))]
ATTN_PARAMS = [pytest.param(c, *k.values, id=f"{'x'.join(map(str, c[:6]))}-c{int(c[6])}-w{c[7]}-{k.id}") for c, k in ATTN_CASES]


def _with_nwaves(L, nw, fn):
    assert L.lib().sage_set_tuning(0, nw) == 0
    try:
        return fn()
    finally:
        L.lib().sage_set_tuning(0, 0)


@pytest.mark.parametrize("cfg,kinds", ATTN_PARAMS)
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_attn_qk_int8(L, pv, cfg, kinds):
    """sage_attn_qk_int8_pv_f16 / _f8: q8, k8, v (or the FP8 image) and o as views; causal and not; 4 and 8 waves."""
    from oracle import sage_oracle as O
    B, Hq, Hk, M, N, D, causal, nw = cfg
    ops = memo(("ops", cfg[:6]), [], lambda: _operands(O, cfg, 20))
    vname = "v" if pv == "fp16" else "v_fp8"
    kinds = {(vname if a == "v" else a): k for a, k in kinds.items()}

    def call(t):
        lse, qs, ks = Dense((B, Hq, M)), ops["qs"].to(DEV), ops["ks"].to(DEV)
        if pv == "fp16":
            st = L.lib().sage_attn_qk_int8_pv_f16(d4(L, t["q8"]), d4(L, t["k8"]), d4(L, t["v"]), L.SAGE_F16, d4(L, t["o"]),
                                                  L.SAGE_F16, qs.data_ptr(), ks.data_ptr(), None, lse.ptr(), B, Hq, Hk, M, N, D,
                                                  int(causal), 3, 128, 32, D ** -0.5, 0, _stream())
        else:
            vs = ops["v_scale"].to(DEV)
            st = L.lib().sage_attn_qk_int8_pv_f8(d4(L, t["q8"]), d4(L, t["k8"]), d4(L, t["v_fp8"]), d4(L, t["o"]), L.SAGE_F16,
                                                 qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), None, lse.ptr(), B, Hq, Hk, M, N, D,
                                                 int(causal), 3, 128, 32, D ** -0.5, 0, _stream())
        assert st == 0, st
        torch.cuda.synchronize()
        return {"lse": lse}
    ins = {"q8": ops["q8"], "k8": ops["k8"], vname: ops[vname]}
    got, lg = _with_nwaves(L, nw, lambda: run_both(call, ins, {"o": ((B, Hq, M, D), F16)}, kinds))
    oo, ol2 = memo(("attn", cfg[:7], pv), lg.values(), lambda: _attn_oracle(O, lg, ops, cfg, pv))
    _check_attn(got, oo, ol2 / LOG2E, pv)


FUSED_ALL = {"q": "seq_slice_nhd", "k8": "packed_hnd", "v": "kv_cache", "o": "row_padded"}
FUSED_PARAMS = [pytest.param(c, *k.values, id=f"{'x'.join(map(str, c[:6]))}-c{int(c[6])}-w{c[7]}-{k.id}")
                for c in ATTN_CFGS for k in arg_cases(["q", "k8", "v"], ["o"], FUSED_ALL)]


@pytest.mark.parametrize("cfg,kinds", FUSED_PARAMS)
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_attn_fusedq(L, pv, cfg, kinds):
    """sage_attn_fusedq_pv_f16 / _f8: the fp16 query tensor as a view (NaN / Inf around it), quantized in the prologue;
    the LSE is the final natural-log one (km given)."""
    from oracle import sage_oracle as O
    B, Hq, Hk, M, N, D, causal, nw = cfg
    ops = memo(("ops", cfg[:6]), [], lambda: _operands(O, cfg, 20))
    vname = "v" if pv == "fp16" else "v_fp8"
    kinds = {(vname if a == "v" else a): k for a, k in kinds.items()}

    def call(t):
        lse, ks, km = Dense((B, Hq, M)), ops["ks"].to(DEV), ops["km"].to(DEV)
        if pv == "fp16":
            st = L.lib().sage_attn_fusedq_pv_f16(d4(L, t["q"]), L.SAGE_F16, d4(L, t["k8"]), d4(L, t["v"]), L.SAGE_F16,
                                                 d4(L, t["o"]), L.SAGE_F16, ks.data_ptr(), km.data_ptr(), None, lse.ptr(), B, Hq,
                                                 Hk, M, N, D, int(causal), 3, 32, D ** -0.5, _stream())
        else:
            vs = ops["v_scale"].to(DEV)
            st = L.lib().sage_attn_fusedq_pv_f8(d4(L, t["q"]), L.SAGE_F16, d4(L, t["k8"]), d4(L, t["v_fp8"]), d4(L, t["o"]),
                                                L.SAGE_F16, ks.data_ptr(), km.data_ptr(), vs.data_ptr(), None, lse.ptr(), B, Hq,
                                                Hk, M, N, D, int(causal), 3, 32, D ** -0.5, _stream())
        assert st == 0, st
        torch.cuda.synchronize()
        return {"lse": lse}
    ins = {"q": ops["q"], "k8": ops["k8"], vname: ops[vname]}
    got, lg = _with_nwaves(L, nw, lambda: run_both(call, ins, {"o": ((B, Hq, M, D), F16)}, kinds))

    def oracle():
        q8, qs, _, _ = O.per_thread_int8(lg["q"], ops["k"], ops["km"].unsqueeze(2))
        oo, ol2 = _attn_oracle(O, lg, ops, cfg, pv, q8=q8, qs=qs)
        return oo, ol2 / LOG2E + O.lse_correction(lg["q"], ops["km"].unsqueeze(2)) * D ** -0.5
    oo, ol = memo(("fusedq", cfg[:7], pv), lg.values(), oracle)
    _check_attn(got, oo, ol, pv, lse_is_base2=False)


# ---- attention with a mask ------------------------------------------------------------------------------------------------
def _mask_view(kind, B, Hq, M, N, seed):
    """A [B,Hq,M,N] mask view: broadcast over the batch (stride 0), a window of a larger [Hq, M+7, N+29] parent whose other
    elements are poison -- "allowed" (1) for the bool kind, so a read outside the window lets a foreign key in; NaN for the
    additive kind.  Every 16th row keeps no key (<= 1/8 of the rows; undefined in the reference, excluded below)."""
    g = torch.Generator().manual_seed(seed)
    allowed = torch.rand((Hq, M, N), generator=g) > 0.4
    allowed[:, :, 0] = True
    allowed[:, ::16] = False
    if kind == 1:
        parent = torch.ones((Hq, M + 7, N + 29), dtype=torch.bool)
        vals = allowed
    else:
        parent = torch.full((Hq, M + 7, N + 29), float("nan"), dtype=F16)
        vals = torch.where(allowed, torch.randn((Hq, M, N), generator=g) * 0.5, torch.tensor(-1.0e4)).to(F16)
    parent[:, 3:3 + M, 11:11 + N] = vals
    view = parent[:, 3:3 + M, 11:11 + N].unsqueeze(0).expand(B, Hq, M, N)
    return parent, view, allowed.unsqueeze(0).expand(B, Hq, M, N)


MASK_ALL = {"q8": "head_batch_slice", "k8": "seq_slice", "v": "packed_nhd", "o": "kv_cache"}


@pytest.mark.parametrize("kinds", [pytest.param({}, id="mask-only"), pytest.param({"k8": "kv_cache"}, id="k8-kv_cache"),
                                   pytest.param({"v": "seq_slice"}, id="v-seq_slice"), pytest.param({"q8": "packed_hnd"}, id="q8-packed_hnd"),
                                   pytest.param({"o": "row_padded"}, id="o-row_padded"), pytest.param(MASK_ALL, id="all")])
@pytest.mark.parametrize("mask_kind", [1, 2])
@pytest.mark.parametrize("cfg", [(2, 4, 2, 200, 333, 64, False, 8), (2, 2, 2, 150, 260, 128, False, 4)], ids=str)
def test_attn_masked(L, cfg, mask_kind, kinds):
    """sage_attn_qk_int8_pv_f16_masked: the mask itself is a strided view with a broadcast dimension and poison around it
    in BOTH runs (the contiguous run gets a dense copy).  Bounds of test_masked.test_masked_hip_vs_reference (|do| < 4e-3;
    base-2 LSE within conftest.LSE2_TOL_ROUNDED_P at head_dim 64, LSE2_TOL_FP32_P at 128), rows with no allowed key
    excluded as there."""
    from oracle import sage_oracle as O
    B, Hq, Hk, M, N, D, _, nw = cfg
    ops = memo(("ops", cfg[:6]), [], lambda: _operands(O, cfg, 20))
    parent, mview, allowed = _mask_view(mask_kind, B, Hq, M, N, 9)
    has_keys = allowed.any(dim=-1)
    assert int((~has_keys).sum()) * 8 <= has_keys.numel()
    parent_d = parent.to(DEV)
    strided = parent_d.as_strided(mview.size(), mview.stride(), mview.storage_offset())
    masks = [strided, strided.contiguous()]

    def call(t):
        m = masks.pop(0)
        lse, qs, ks = Dense((B, Hq, M)), ops["qs"].to(DEV), ops["ks"].to(DEV)
        st = L.lib().sage_attn_qk_int8_pv_f16_masked(d4(L, t["q8"]), d4(L, t["k8"]), d4(L, t["v"]), L.SAGE_F16, d4(L, t["o"]),
                                                     L.SAGE_F16, qs.data_ptr(), ks.data_ptr(), m.data_ptr(), mask_kind,
                                                     (ctypes.c_int64 * 4)(*m.stride()), lse.ptr(), B, Hq, Hk, M, N, D, 3, 128, 32,
                                                     D ** -0.5, 0, _stream())
        assert st == 0, st
        torch.cuda.synchronize()
        return {"lse": lse}
    ins = {"q8": ops["q8"], "k8": ops["k8"], "v": ops["v"]}
    got, lg = _with_nwaves(L, nw, lambda: run_both(call, ins, {"o": ((B, Hq, M, D), F16)}, kinds))
    assert torch.equal(V.raw_bytes(parent_d).cpu(), V.raw_bytes(parent)), "the mask's parent was modified"
    oo, ol2 = memo(("masked", cfg[:6], mask_kind), lg.values(), lambda: _attn_oracle(O, lg, ops, cfg, "fp16", mask=mview.contiguous()))
    sel = has_keys
    assert torch.isfinite(got["o"][sel]).all() and torch.isfinite(got["lse"][sel]).all()
    assert (got["o"].float() - oo.float())[sel].abs().max() < 4e-3
    assert (got["lse"] - ol2)[sel].abs().max() < (LSE2_TOL_ROUNDED_P if D == 64 else LSE2_TOL_FP32_P)


# ---- packed variable-length sequences -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [pytest.param({a: k for a in "q k v q8 k8 o".split()}, id=f"all-{k}") for k in ("packed_nhd", "seq_slice_nhd")]
                         + [pytest.param({a: k}, id=f"{a}-{k}") for k in ("packed_nhd", "seq_slice_nhd") for a in "q k v q8 k8 o".split()])
@pytest.mark.parametrize("causal", [False, True])
def test_varlen(L, causal, kinds):
    """sage_quant_qk_int8_varlen (Q and K) feeding sage_attn_qk_int8_pv_f16_varlen: packed [T,H,D] tensors as the q / k / v
    of a packed QKV projection (stride_n = 3HD) and as a slice of a longer packed buffer; the int8 intermediates are views
    too (written by one call, read by the next).  (b) as test_varlen.test_varlen_hip_vs_reference_and_oracle: 4 fp16 ulps."""
    from oracle import sage_oracle as O
    lens = [77, 200, 5, 141]
    cu = torch.tensor([0, 77, 277, 282, 423], dtype=torch.int32)
    T, Hq, Hk, D, nseq, mx = 423, 4, 2, 64, 4, 200
    q = V.random_values((1, Hq, T, D), F16, 30)
    k = V.random_values((1, Hk, T, D), F16, 31, channel_bias=1.0)
    v = V.random_values((1, Hk, T, D), F16, 32)
    sm = D ** -0.5

    def call(t):
        cu_d = cu.to(DEV)
        km = t["k"].cpu()[0].transpose(0, 1).float().mean(dim=0, keepdim=True).to(F16).contiguous().to(DEV)  # [1,Hk,D], core.py:461
        # [num_seqs, H, G(max_seqlen)]: a sequence writes the scales of its own blocks only
        qs, ks = Dense((nseq, Hq, (mx + 127) // 128), full=False), Dense((nseq, Hk, (mx + 63) // 64), full=False)
        lib = L.lib()
        assert lib.sage_quant_qk_int8_varlen(d4(L, t["q"]), 0, cu_d.data_ptr(), nseq, Hq, mx, D, None, d4(L, t["q8"]), qs.ptr(), 1,
                                             0, 128, 128, float(sm * 1.44269504), 0, _stream()) == 0
        assert lib.sage_quant_qk_int8_varlen(d4(L, t["k"]), 0, cu_d.data_ptr(), nseq, Hk, mx, D, km.data_ptr(), d4(L, t["k8"]),
                                             ks.ptr(), 1, 1, 64, 64, 1.0, 0, _stream()) == 0
        assert lib.sage_attn_qk_int8_pv_f16_varlen(d4(L, t["q8"]), d4(L, t["k8"]), d4(L, t["v"]), 0, d4(L, t["o"]), 0, qs.ptr(),
                                                   ks.ptr(), cu_d.data_ptr(), cu_d.data_ptr(), nseq, Hq, Hk, mx, mx, D, int(causal),
                                                   1, 128, 128, sm, 1, _stream()) == 0
        torch.cuda.synchronize()
        return {"qs": qs, "ks": ks}
    outs = {"q8": ((1, Hq, T, D), I8), "k8": ((1, Hk, T, D), I8), "o": ((1, Hq, T, D), F16)}
    got, lg = run_both(call, {"q": q, "k": k, "v": v}, outs, kinds)
    pk = lambda x: x[0].transpose(0, 1)  # noqa: E731  [1,H,T,D] -> packed [T,H,D]
    oo = memo(("varlen", causal), lg.values(),
              lambda: O.sageattn_varlen_oracle(pk(lg["q"]), pk(lg["k"]), pk(lg["v"]), cu, cu, is_causal=causal)).float()
    o = pk(got["o"]).float()
    assert torch.isfinite(o).all()
    for sc, blk in ((got["qs"], 128), (got["ks"], 64)):  # a sequence's own blocks finite, the other slots never written
        used = torch.tensor([[g < (n + blk - 1) // blk for g in range(sc.shape[2])] for n in lens]).unsqueeze(1).expand(sc.shape)
        assert torch.isfinite(sc[used]).all() and torch.isnan(sc[~used]).all()
    assert ((o - oo).abs() <= 4 * 2.0 ** -10 * oo.abs().clamp(min=0.25)).all()
    # the int8 tensors bit-exact against the oracle's per-sequence quantizer (test_varlen.test_varlen_oracle_vs_reference)
    km = pk(lg["k"]).float().mean(dim=0, keepdim=True).to(F16)
    for s in range(nseq):
        a, b = int(cu[s]), int(cu[s + 1])
        r = O.per_block_int8(pk(lg["q"])[a:b].unsqueeze(0), pk(lg["k"])[a:b].unsqueeze(0), km.unsqueeze(0), sm_scale=sm, tensor_layout="NHD")
        assert torch.equal(r[0][0], pk(got["q8"])[a:b]) and torch.equal(r[2][0], pk(got["k8"])[a:b])


# ---- the one-call operators -----------------------------------------------------------------------------------------------
OP_CFGS = [
    # (B, Hq, Hk, M, N, D, causal, dtype, gran, nwaves)
    (2, 4, 2, 200, 333, 64, False, F16, 3, 0),
    (2, 2, 2, 333, 333, 128, True, BF16, 2, 4),
]
OP_LONG = (1, 2, 1, 4200, 4133, 128, True, F16, 3, 8)
OP_ALL = {"q": "packed_nhd", "k": "kv_cache", "v": "seq_slice", "o": "head_batch_slice"}
OP_PARAMS = [pytest.param(c, *k.values, id=f"{'x'.join(map(str, c[:6]))}-c{int(c[6])}-{str(c[7])[6:]}-g{c[8]}-{k.id}")
             for c in OP_CFGS for k in arg_cases(["q", "k", "v"], ["o"], OP_ALL)] + [pytest.param(OP_LONG, OP_ALL, id="all-long")]


@pytest.mark.parametrize("cfg,kinds", OP_PARAMS)
@pytest.mark.parametrize("pv", ["fp16", "fp8"])
def test_one_call_operator(L, pv, cfg, kinds):
    """sage_sageattn_pv_f16 / _f8 -- what a user's tensors reach first -- with q, k, v, o as views of every kind.  (b): fp16
    as test_edge_shapes_vs_oracle (2e-3 / 0.06, LSE 2e-3); bf16 as test_randomized_sweep_vs_oracle (1.6e-2 / 0.07, LSE 3e-3)."""
    from oracle import sage_oracle as O
    B, Hq, Hk, M, N, D, causal, dt, gran, nw = cfg
    q = V.random_values((B, Hq, M, D), dt, 40)
    k = V.random_values((B, Hk, N, D), dt, 41, channel_bias=1.5)
    v = V.random_values((B, Hk, N, D), dt, 42)
    opts = L.OpOpts(gran, 32, 1, -1, nw)
    lib = L.lib()
    nbytes = lib.sage_sageattn_workspace_bytes(int(pv == "fp8"), B, Hq, Hk, M, N, D, 1, opts)
    assert nbytes > 0

    def call(t):
        lse, ws = Dense((B, Hq, M)), ws_for(nbytes)
        args = (d4(L, t["q"]), d4(L, t["k"]), d4(L, t["v"]), code(L, dt), d4(L, t["o"]), lse.ptr(), B, Hq, Hk, M, N, D, int(causal),
                D ** -0.5)
        if pv == "fp16":
            st = lib.sage_sageattn_pv_f16(*args, opts, ws.data_ptr(), nbytes, _stream())
        else:
            st = lib.sage_sageattn_pv_f8(*args, 448.0, opts, ws.data_ptr(), nbytes, _stream())
        assert st == 0, st
        torch.cuda.synchronize()
        return {"lse": lse}
    got, lg = run_both(call, {"q": q, "k": k, "v": v}, {"o": ((B, Hq, M, D), dt)}, kinds)
    oo, ol = memo(("op", cfg[:9], pv), lg.values(),
                  lambda: O.sageattn_oracle(lg["q"], lg["k"], lg["v"], is_causal=causal, pv=pv, return_lse=True,
                                            qk_quant_gran="per_thread" if gran == 3 else "per_warp"))
    assert torch.isfinite(got["o"]).all() and torch.isfinite(got["lse"]).all()
    tol = {("fp16", F16): 2e-3, ("fp16", BF16): 1.6e-2, ("fp8", F16): 0.06, ("fp8", BF16): 0.07}[(pv, dt)]
    assert (got["o"].float() - oo.float()).abs().max() < tol
    assert (got["lse"] - ol).abs().max() < (2e-3 if dt == F16 else 3e-3)


# ---- the public Python operators ------------------------------------------------------------------------------------------
def _public_ops(sa):
    return {"sageattn": sa.sageattn, "fp16_cuda": sa.sageattn_qk_int8_pv_fp16_cuda, "fp8_cuda": sa.sageattn_qk_int8_pv_fp8_cuda,
            "fp16_triton": sa.sageattn_qk_int8_pv_fp16_triton}


PUBLIC_KINDS = ("packed_nhd", "packed_hnd", "kv_cache", "seq_slice")


@pytest.mark.parametrize("D", [64, 128, 40, 96])
@pytest.mark.parametrize("kind", PUBLIC_KINDS)
@pytest.mark.parametrize("op", ["sageattn", "fp16_cuda", "fp8_cuda", "fp16_triton", "fp16_triton_mask"])
def test_public_operators(L, op, kind, D):
    """sageattn, sageattn_qk_int8_pv_{fp16,fp8}_cuda, sageattn_qk_int8_pv_fp16_triton (with and without attn_mask) on q, k, v
    that are all views of one kind (padded head dims 40 and 96 included): (a) against contiguous copies, (b) / (c) with
    the bounds of test_edge_shapes_vs_oracle; with a mask those of test_masked.test_masked_api_end_to_end (0.08 against
    exact masked attention)."""
    import sageattention_amd as sa
    from oracle import sage_oracle as O
    B, Hq, Hk, M, N = 2, 4, 2, 200, 333
    dt = BF16 if D == 96 else F16
    q = V.make_input(kind, (B, Hq, M, D), dt, seed=50).to(DEV)
    k = V.make_input(kind, (B, Hk, N, D), dt, seed=51, channel_bias=1.5).to(DEV)
    v = V.make_input(kind, (B, Hk, N, D), dt, seed=52).to(DEV)
    layout = q.layout
    fn = _public_ops(sa)[op.replace("_mask", "")]
    kw = dict(tensor_layout=layout, return_lse=True)
    if op.endswith("_mask"):
        mask = torch.rand((M, N), generator=torch.Generator().manual_seed(4)) > 0.4
        mask[:, 0] = True
        kw["attn_mask"] = mask.to(DEV)
    o, lse = fn(q.arg(), k.arg(), v.arg(), **kw)
    o2, lse2 = fn(q.arg().contiguous(), k.arg().contiguous(), v.arg().contiguous(), **kw)
    torch.cuda.synchronize()
    assert o.shape == q.arg().shape and _same_bits(o.cpu(), o2.cpu()) and _same_bits(lse.cpu(), lse2.cpu())
    assert q.parent_unchanged() and k.parent_unchanged() and v.parent_unchanged()
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    oh = (o if layout == "HND" else o.transpose(1, 2)).cpu().float()
    if op.endswith("_mask"):
        s = (q.logical.float() @ k.logical.float().repeat_interleave(Hq // Hk, dim=1).transpose(2, 3)) * D ** -0.5
        ref = torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ v.logical.float().repeat_interleave(Hq // Hk, dim=1)
        assert (oh - ref).abs().max() < 0.08
        return
    pv = "fp8" if op == "fp8_cuda" else "fp16" if op != "sageattn" else sa.core.dispatch_pv(q.arg(), k.arg(), layout, False)
    oo, ol = O.sageattn_oracle(q.logical, k.logical, v.logical, pv=pv, return_lse=True)
    tol = {("fp16", F16): 2e-3, ("fp16", BF16): 1.6e-2, ("fp8", F16): 0.06, ("fp8", BF16): 0.07}[(pv, dt)]
    assert (oh - oo.float()).abs().max() < tol
    assert (lse.cpu() - ol).abs().max() < (2e-3 if dt == F16 else 3e-3)


@pytest.mark.parametrize("kind", ["packed_nhd", "seq_slice_nhd"])
def test_public_varlen(L, kind):
    """sageattn_varlen on packed [T,H,D] views (a packed QKV projection; a slice of a longer buffer), head_dim 64 and 96."""
    import sageattention_amd as sa
    from oracle import sage_oracle as O
    cu = torch.tensor([0, 77, 277, 282, 423], dtype=torch.int32)
    for D, dt in ((64, F16), (96, BF16)):
        q, k, v = (V.make_input(kind, (1, 4 if i == 0 else 2, 423, D), dt, seed=60 + i, channel_bias=float(i == 1)).to(DEV) for i in range(3))
        pk = lambda c: c.view[0].transpose(0, 1)  # noqa: E731
        o = sa.sageattn_varlen(pk(q), pk(k), pk(v), cu.to(DEV), cu.to(DEV), 200, 200)
        o2 = sa.sageattn_varlen(pk(q).contiguous(), pk(k).contiguous(), pk(v).contiguous(), cu.to(DEV), cu.to(DEV), 200, 200)
        torch.cuda.synchronize()
        assert _same_bits(o.cpu(), o2.cpu()) and torch.isfinite(o).all()
        assert q.parent_unchanged() and k.parent_unchanged() and v.parent_unchanged()
        oo = O.sageattn_varlen_oracle(pk(q).cpu(), pk(k).cpu(), pk(v).cpu(), cu, cu).float()
        if dt == F16:   # test_varlen.test_varlen_hip_vs_reference_and_oracle
            assert ((o.cpu().float() - oo).abs() <= 4 * 2.0 ** -10 * oo.abs().clamp(min=0.25)).all()
        else:           # test_varlen.test_varlen_cross_lengths_bf16_int64
            assert (o.cpu().float() - oo).abs().max() < 1.6e-2


# ---- views the C ABI refuses, at the Python boundary ----------------------------------------------------------------------
def _refused_view(which, shape, dt, seed):
    """``x[..., 4:68]`` (base only 8-byte aligned) or a row stride of D + 4 elements, poison around the values."""
    B, H, N, D = shape
    vals = V.random_values(shape, dt, seed, channel_bias=1.0)
    wide = torch.full((B, H, N, D + (8 if which == "offset" else 4)), float("nan"), dtype=dt)
    view = wide[..., 4:4 + D] if which == "offset" else wide[..., :D]
    view.copy_(vals)
    wide = wide.to(DEV)
    return wide[..., 4:4 + D] if which == "offset" else wide[..., :D]


@pytest.mark.parametrize("which", ["offset", "stride"])
@pytest.mark.parametrize("arg", ["q", "k", "v"])
@pytest.mark.parametrize("op", ["sageattn", "fp16_cuda", "fp8_cuda", "fp16_triton"])
def test_public_operators_accept_what_the_c_abi_refuses(L, op, arg, which):
    """The reference takes every tensor with a contiguous last dim (core.py:592-601); the C ABI wants 16-byte aligned rows
    and returns SAGE_ERR_INVALID_ARGUMENT otherwise.  The Python operators pass such a view as a contiguous copy: same bits
    as on contiguous tensors.  The C ABI itself stays strict."""
    import sageattention_amd as sa
    B, H, N, D = 2, 2, 200, 64
    ts = {n: (_refused_view(which, (B, H, N, D), F16, 70 + i) if n == arg else V.random_values((B, H, N, D), F16, 70 + i, channel_bias=1.0).to(DEV))
          for i, n in enumerate("qkv")}
    bad = ts[arg]
    assert bad.stride(-1) == 1 and not (bad.data_ptr() % 16 == 0 and bad.stride(2) % 8 == 0)
    ws = ws_for(1 << 22)
    opts = L.OpOpts(3, 32, 1, -1, 0)
    o = torch.empty((B, H, N, D), dtype=F16, device=DEV)
    assert L.lib().sage_sageattn_pv_f16(*(d4(L, ts[n]) for n in "qkv"), 0, d4(L, o), None, B, H, H, N, N, D, 0, 0.125, opts,
                                        ws.data_ptr(), ws.numel(), _stream()) == -1
    fn = _public_ops(sa)[op]
    o, lse = fn(ts["q"], ts["k"], ts["v"], return_lse=True)
    o2, lse2 = fn(*(ts[n].contiguous() for n in "qkv"), return_lse=True)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all() and _same_bits(o.cpu(), o2.cpu()) and _same_bits(lse.cpu(), lse2.cpu())


def test_public_varlen_accepts_what_the_c_abi_refuses(L):
    import sageattention_amd as sa
    cu = torch.tensor([0, 77, 277], dtype=torch.int32, device=DEV)
    for which in ("offset", "stride"):
        q, k, v = (_refused_view(which, (1, 2, 277, 64), F16, 80 + i)[0].transpose(0, 1) for i in range(3))
        o = sa.sageattn_varlen(q, k, v, cu, cu, 200, 200)
        o2 = sa.sageattn_varlen(q.contiguous(), k.contiguous(), v.contiguous(), cu, cu, 200, 200)
        assert torch.isfinite(o).all() and _same_bits(o.cpu(), o2.cpu())


# ---- contiguous-by-contract arrays: exact length ----------------------------------------------------------------------------
def test_merges_and_finish_lse_write_their_exact_length(L):
    """sage_merge_attn_states, _multi, _multi_ex and sage_finish_lse take plain contiguous arrays: every output lies between
    sentinel guards (rows = 1001, not a multiple of any block size) and must be written completely and nowhere else."""
    rows, D, lib = 1001, 64, L.lib()
    g = torch.Generator().manual_seed(3)
    ob = [torch.randn((rows, D), generator=g).to(F16).to(DEV) for _ in range(3)]
    lb = [(torch.randn((rows,), generator=g) * 3).to(DEV) for _ in range(3)]
    oa, la = Dense((rows, D)), Dense((rows,))
    oa.t.copy_(torch.randn((rows, D), generator=g)); la.t.copy_(torch.randn((rows,), generator=g))
    assert lib.sage_merge_attn_states(oa.ptr(), la.ptr(), ob[0].data_ptr(), 0, lb[0].data_ptr(), rows, D, _stream()) == 0
    torch.cuda.synchronize()
    o1, l1 = oa.result("o_acc"), la.result("lse_acc")
    assert torch.isfinite(o1).all() and torch.isfinite(l1).all()
    op = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ob])
    lp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in lb])
    ref_l = torch.logsumexp(torch.stack(lb), dim=0).cpu()
    for ex in (False, True):
        oo, lo = Dense((rows, D), F16), Dense((rows,))
        if ex:
            st = lib.sage_merge_attn_states_multi_ex(op, lp, 3, 0, oo.ptr(), lo.ptr(), rows, D, 1.0, None, 0.0, _stream())
        else:
            st = lib.sage_merge_attn_states_multi(op, lp, 3, 0, oo.ptr(), lo.ptr(), rows, D, _stream())
        assert st == 0
        torch.cuda.synchronize()
        o, l = oo.result("o_out"), lo.result("lse_out")
        assert torch.isfinite(o).all() and (l - ref_l).abs().max() < 1e-5   # test_gpu_parity.test_multiway_merge_vs_torch
    out = Dense((rows,))
    assert lib.sage_finish_lse(lb[0].data_ptr(), lb[1].data_ptr(), 0.125, out.ptr(), rows, _stream()) == 0
    torch.cuda.synchronize()
    want = lb[0].cpu() / LOG2E + lb[1].cpu() * 0.125
    assert (out.result("lse_out") - want).abs().max() < 1e-5


# ---- tile-major exchange buffers ----------------------------------------------------------------------------------------------
def _tile_view(parent, base, B, H, N, rows, row_len, sb, sh, st, sn):
    """[B,H,T,rows,row_len] view of a flat parent: tile t of (b,h) at base + b*sb + h*sh + t*st, its rows sn apart."""
    T = (N + 63) // 64
    view = parent.as_strided((B, H, T, rows, row_len), (sb, sh, st, sn, 1), base)
    return view, T


def test_tile_major_entry_points(L):
    """sage_quant_k_int8_kvtiles, sage_quant_v_fp8_apply and sage_attn_qk_int8_pv_{f16,f8}_kvtiles with the tile-major buffers
    as windows of larger poisoned buffers: tile strides larger than a tile, rows longer than a row, a ragged last tile.  The
    quantizers' bytes against the oracle (bit-exact, as test_gather_gpu.test_tile_major_quantizers_are_bit_identical_to_the_
    dense_ones pins them to the dense quantizers) and nothing written around them; the attention calls bit-identical to the
    dense entry points on contiguous copies, and within 2e-3 / 0.06 (LSE 2e-3) of the oracle as test_edge_shapes_vs_oracle."""
    from oracle import sage_oracle as O
    B, Hq, Hk, M, N, D = 2, 4, 2, 200, 300, 128
    cfg = (B, Hq, Hk, M, N, D, False)
    ops = memo(("ops", cfg[:6]), [], lambda: _operands(O, cfg, 20))
    T, lib, st_ = (N + 63) // 64, L.lib(), _stream()
    k, v, km = ops["k"].to(DEV), ops["v"].to(DEV), ops["km"].to(DEV)
    # K: rows of D + 16 bytes, tiles 1.5 tiles apart, heads and batches after all tiles
    sn, tile = D + 16, 96 * (D + 16)
    sh, sb, base = T * tile + 64, Hk * (T * tile + 64) + 256, 48
    kbuf = V.sentinel((base + B * sb + 999,), I8).to(DEV)
    k8v, _ = _tile_view(kbuf, base, B, Hk, N, 64, D, sb, sh, tile, sn)
    ks = Dense((B, Hk, T * 4))
    out = L.SageTensor(kbuf.data_ptr() + base, sb, sh, sn)
    assert lib.sage_quant_k_int8_kvtiles(d4(L, k), 0, B, Hk, N, D, km.data_ptr(), out, tile, ks.ptr(),
                                         (ctypes.c_int64 * 3)(Hk * T * 4, T * 4, 4), 3, 0, st_) == 0
    torch.cuda.synchronize()
    got_k = k8v.reshape(B, Hk, T * 64, D)[:, :, :N].cpu()
    assert torch.equal(got_k, ops["k8"]) and torch.equal(ks.result("k_scale"), ops["ks"])
    inside = V.byte_mask(kbuf.cpu().as_strided(k8v.size(), k8v.stride(), base), kbuf.cpu())
    raw = V.raw_bytes(kbuf).cpu()
    tail = V.byte_mask(kbuf.cpu().as_strided((B, Hk, 1, 64 - N % 64, D), k8v.stride(), base + (T - 1) * tile + (N % 64) * sn), kbuf.cpu())
    assert (raw[~inside | tail] == 0x80).all(), "sage_quant_k_int8_kvtiles wrote outside its rows"
    # V -> FP8 image, tile-major: channel rows of 80 bytes, token blocks 1.25 blocks apart
    vsn, vtile = 80, 160 * D
    vsh, vsb = T * vtile + 128, Hk * (T * vtile + 128) + 512
    vbuf = V.sentinel((base + B * vsb + 777,), F8).to(DEV)
    v8v, _ = _tile_view(vbuf, base, B, Hk, N, D, 64, vsb, vsh, vtile, vsn)
    coef = torch.stack([torch.zeros(B, Hk, D), O._ieee_div(448.0, ops["v"].float().abs().amax(2))], dim=2).contiguous().to(DEV)
    vout = L.SageTensor(vbuf.data_ptr() + base, vsb, vsh, vsn)
    assert lib.sage_quant_v_fp8_apply(d4(L, v), 0, B, Hk, N, D, vout, vtile, coef.data_ptr(), st_) == 0
    torch.cuda.synchronize()
    got_v = v8v.permute(0, 1, 3, 2, 4).reshape(B, Hk, D, T * 64).cpu().view(torch.uint8)
    assert torch.equal(got_v, ops["v_fp8"].view(torch.uint8)), "FP8 image (zero columns past N included) differs from the oracle's"
    vin = V.byte_mask(vbuf.cpu().as_strided(v8v.size(), v8v.stride(), base), vbuf.cpu())
    assert (V.raw_bytes(vbuf).cpu()[~vin] == 0xFF).all(), "sage_quant_v_fp8_apply wrote outside its image"
    # fp16 V tile-major inside NaN / Inf
    fsn, ftile = D + 8, 80 * (D + 8)
    fsh, fsb = T * ftile + 64, Hk * (T * ftile + 64) + 128
    fbuf = V.poisoned((base + B * fsb + 555,), F16, 5)
    fv = fbuf.as_strided((B, Hk, T, 64, D), (fsb, fsh, ftile, fsn, 1), base)
    for t in range(T):
        n = min(64, N - 64 * t)
        fv[:, :, t, :n] = ops["v"][:, :, 64 * t:64 * t + n]
    fbuf = fbuf.to(DEV)
    q8, qs, vs = ops["q8"].to(DEV), ops["qs"].to(DEV), ops["v_scale"].to(DEV)
    before_k, before_v = V.raw_bytes(kbuf).clone(), V.raw_bytes(vbuf).clone()
    for pv in ("fp16", "fp8"):
        res = []
        for tiled in (True, False):
            o, lse = V.make_output("head_batch_slice" if tiled else "contiguous", (B, Hq, M, D), F16).to(DEV), Dense((B, Hq, M))
            if tiled:
                kd = L.SageTensor(kbuf.data_ptr() + base, sb, sh, sn)
                vd = (L.SageTensor(fbuf.data_ptr() + 2 * base, fsb, fsh, fsn) if pv == "fp16" else
                      L.SageTensor(vbuf.data_ptr() + base, vsb, vsh, vsn))
                lay = L.KvLayout(tile, ftile if pv == "fp16" else vtile, 0, 0, 0)
                if pv == "fp16":
                    r = lib.sage_attn_qk_int8_pv_f16_kvtiles(d4(L, q8), kd, vd, 0, d4(L, o.view), 0, qs.data_ptr(), ks.ptr(), lay,
                                                             lse.ptr(), B, Hq, Hk, M, N, D, 0, 3, 128, 32, D ** -0.5, st_)
                else:
                    r = lib.sage_attn_qk_int8_pv_f8_kvtiles(d4(L, q8), kd, vd, d4(L, o.view), 0, qs.data_ptr(), ks.ptr(), vs.data_ptr(),
                                                            lay, lse.ptr(), B, Hq, Hk, M, N, D, 0, 3, 128, 32, D ** -0.5, st_)
            else:
                k8d, ksd = ops["k8"].to(DEV), ops["ks"].to(DEV)
                if pv == "fp16":
                    r = lib.sage_attn_qk_int8_pv_f16(d4(L, q8), d4(L, k8d), d4(L, v), 0, d4(L, o.view), 0, qs.data_ptr(), ksd.data_ptr(),
                                                     None, lse.ptr(), B, Hq, Hk, M, N, D, 0, 3, 128, 32, D ** -0.5, 0, st_)
                else:
                    v8d = ops["v_fp8"].to(DEV)
                    r = lib.sage_attn_qk_int8_pv_f8(d4(L, q8), d4(L, k8d), d4(L, v8d), d4(L, o.view), 0, qs.data_ptr(), ksd.data_ptr(),
                                                    vs.data_ptr(), None, lse.ptr(), B, Hq, Hk, M, N, D, 0, 3, 128, 32, D ** -0.5, 0, st_)
            assert r == 0, (pv, tiled, r)
            torch.cuda.synchronize()
            assert o.outside_untouched() and o.all_written()
            res.append((o.view.contiguous().cpu(), lse.result("lse")))
        assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1]), pv
        lg = {"q8": ops["q8"], "k8": ops["k8"], "v": ops["v"], "v_fp8": ops["v_fp8"]}
        oo, ol2 = _attn_oracle(O, lg, ops, cfg, pv)
        _check_attn({"o": res[0][0], "lse": res[0][1]}, oo, ol2 / LOG2E, pv)
    assert torch.equal(V.raw_bytes(kbuf), before_k) and torch.equal(V.raw_bytes(vbuf), before_v), "an attention call wrote its K / V"
