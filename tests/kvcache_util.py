"""The rule of the persistent KV cache (include/sageattn_hip_kvcache.h) restated for the tests: which 64-key tiles an append
touches, and -- on the GPU, through entry points that exist without the cache -- the from-scratch quantization that the
valid part of a cache must equal bit for bit."""
import torch


def clamp_len(n, N):
    return min(max(int(n), 0), N)


def touched_tiles(start, length, N):
    """the 64-key tiles ``append`` quantizes for a batch: none without keys, else from the tile that holds row
    min(start, len - 1) to the last tile of len rows (both lengths clamped to [0, N])"""
    s, l = clamp_len(start, N), clamp_len(length, N)
    if l == 0:
        return range(0)
    return range(min(s, l - 1) // 64, (l + 63) // 64)


def touched_v_blocks(start, length, N, D):
    """the 64-token blocks of the V^T image an append may write: the touched tiles, and at head_dim 64 -- a workgroup holds
    two blocks -- the whole block below an odd first tile (the same bytes from unchanged rows)"""
    t = touched_tiles(start, length, N)
    if len(t) == 0 or D == 128:
        return t
    return range(t.start // 2 * 2, t.stop)


def need(start, length, N):
    """rows a batch gains: what ``max_new`` must cover"""
    s, l = clamp_len(start, N), clamp_len(length, N)
    return l - min(s, l)


# ---- GPU: the from-scratch operands ------------------------------------------------------------------------------------------
def hnd(t, layout):
    """the [B,H,N,D] view of k, v or k8, or the [B,H,D,Npad] view of the V^T image"""
    return t if layout == "HND" else t.transpose(1, 2)


def gpb(cache):
    return 4 if cache.qk_quant_gran == "per_thread" else 1


def scratch_k(cache, b, length):
    """sage_quant_qk_int8(k[b, :, :length], mean = km[b], is_key = 1, blk 64, warp 64, the cache's gran and rounding)
    -> (int8 [H, length, D], scales [H, ceil(length/64) * groups])"""
    from sageattention_amd import core
    from sageattention_amd.quant import _quant
    gran, rnd = core._k_pairing(cache.qk_quant_gran)
    x = hnd(cache.k, cache.tensor_layout)[b:b + 1, :, :length]
    k8, ks, _ = _quant(x, "HND", gran, True, 64, 64, 1.0, rnd, mean=cache.km[b:b + 1].contiguous())
    return k8[0], ks[0]


def scratch_v(cache, b, length):
    """sage_quant_v_fp8_apply(v[b, :, :length], v_coef[b]) -> uint8 [H, D, 64 * ceil(length/64)], with the rule's one
    departure from it: where v * coef lies beyond +-448 that call returns the NaN byte (the conversion does not saturate) and
    the cache holds +-448 (0x7E / 0xFE).  A NaN byte anywhere else fails here."""
    from sageattention_amd import _lib as L
    from sageattention_amd.quant import fp8_token_order
    x = hnd(cache.v, cache.tensor_layout)[b:b + 1, :, :length]
    _, H, _, D = x.shape
    npad = (length + 63) // 64 * 64
    out = torch.full((1, H, D, npad), 0xA5, dtype=torch.uint8, device=x.device)
    L.check(L.lib().sage_quant_v_fp8_apply(L.desc(x, "HND"), L.dtype_code(x.dtype), 1, H, length, D, L.desc_vt(out, "HND"), 0,
                                           cache.v_coef[b:b + 1].contiguous().data_ptr(), L.stream_ptr(x.device)),
            "sage_quant_v_fp8_apply")
    out = out[0]
    nan = (out & 0x7F) == 0x7F
    if bool(nan.any()):
        y = torch.zeros((H, D, npad), dtype=torch.float32, device=x.device)
        y[:, :, :length] = (x[0].float() * cache.v_coef[b, :, 1].unsqueeze(1)).transpose(1, 2)   # the kernel's fp32 product
        y = y.view(H, D, npad // 64, 64)[..., fp8_token_order().to(x.device)].reshape(H, D, npad)  # position <- token
        assert bool((y[nan].abs() > 448).all()), "a NaN byte where v * coef is within the range"
        out = torch.where(nan, torch.where(y > 0, 0x7E, 0xFE).to(torch.uint8), out)
    return out


def scratch_operands(cache, lens):
    """the ``kv`` of ``core._splitkv_attn`` rebuilt from scratch for the prefixes ``lens`` (a list) against the cache's frozen
    km / V coefficients: new tensors of the cache's shapes, zero outside the valid part"""
    layout, fp8 = cache.tensor_layout, cache.pv == "fp8"
    k8 = torch.zeros_like(cache.k8)
    ks = torch.zeros_like(cache.k_scale)
    v8 = torch.zeros_like(cache.v8.view(torch.uint8)) if fp8 else None
    for b, n in enumerate(lens):
        if n == 0:
            continue
        rk8, rks = scratch_k(cache, b, n)
        hnd(k8, layout)[b, :, :n] = rk8
        ks[b, :, :rks.shape[1]] = rks
        if fp8:
            rv = scratch_v(cache, b, n)
            hnd(v8, layout)[b, :, :, :rv.shape[2]] = rv
    if fp8:
        return k8, ks, cache.km, v8.view(torch.float8_e4m3fn), cache.v_scale, None
    return k8, ks, cache.km, cache.v, None, None


def assert_valid_state_is_from_scratch(cache, lens):
    """the valid part of the cache -- INT8 rows < len_b, the scales of the tiles below ceil(len_b/64), and for FP8 P.V the
    blocks of the V^T image below it, zero columns included -- equals the from-scratch quantization, bit for bit"""
    layout, g = cache.tensor_layout, gpb(cache)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        nt = (n + 63) // 64
        rk8, rks = scratch_k(cache, b, n)
        assert torch.equal(hnd(cache.k8, layout)[b, :, :n], rk8), ("k8", b, n)
        assert torch.equal(cache.k_scale[b, :, :nt * g], rks), ("k_scale", b, n)
        if cache.pv == "fp8":
            assert torch.equal(hnd(cache.v8.view(torch.uint8), layout)[b, :, :, :nt * 64], scratch_v(cache, b, n)), ("v8", b, n)
