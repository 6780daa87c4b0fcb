"""A V channel that is zero over the whole sequence on the FP8-PV paths.  amax = 0 used to give the coefficient
448 / 0 = inf, an image of (0 - 0) * inf = NaN bytes and a NaN output channel (as the reference does, fused.cu:399) -- on
every padded head dim, and for any caller whose V has a dead channel as soon as the dispatcher picks FP8.  Defined now, like
the other degenerate cases (a batch without keys, a q-block without tiles): image bytes 0x00, v_scale 0, output exactly 0,
and every OTHER channel bit-identical to the same call with the dead channel set to 1.0 (the V scale is per channel and V
is not smoothed)."""
import pytest
import torch

import seqpar_ref as R

pytestmark = pytest.mark.gpu

Z = 5   # the dead channel


def _qkv(D, seed=0, B=1, H=2, N=192):
    g = torch.Generator().manual_seed(seed + D)
    q = torch.randn(B, H, N, D, generator=g).half().cuda()
    k = (torch.randn(B, H, N, D, generator=g) + torch.randn(1, H, 1, D, generator=g)).half().cuda()
    v = torch.randn(B, H, N, D, generator=g).half()
    v[..., Z] = 0
    v1 = v.clone()
    v1[..., Z] = 1.0
    return q, k, v.cuda(), v1.cuda()


def _check_pair(o, lse, o1, lse1, D):
    keep = [d for d in range(D) if d != Z]
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert (o[..., Z] == 0).all()
    assert torch.equal(R.bits(o[..., keep]), R.bits(o1[..., keep]))
    assert torch.equal(R.bits(lse), R.bits(lse1))
    assert (o1[..., Z].float() - 1.0).abs().max() < 0.25           # (the comparison call really attends that channel: ~1)


@pytest.mark.parametrize("D", (64, 128))
def test_zero_channel_quantizers(D):
    """The separate quantizer, the fused K+V pre-pass and its kv_lens twin: image row all 0x00, v_scale 0, the other rows and
    scales those of the V with the channel set to 1.0."""
    import sageattention_amd as sa
    from sageattention_amd import _lib as L
    q, k, v, v1 = _qkv(D)
    keep = [d for d in range(D) if d != Z]
    lens = torch.tensor([150], dtype=torch.int32, device="cuda")
    calls = {
        "separate": lambda x: sa.quant.per_channel_fp8(x, smooth_v=False)[:2],
        "fused": lambda x: sa.quant.kv_prepare_fp8(k, x, "HND", L.GRAN_PER_THREAD, L.ROUND_TRITON)[3:5],
        "kvlen": lambda x: sa.quant.kv_prepare_fp8_kvlen(k, x, lens, "HND", L.GRAN_PER_THREAD, L.ROUND_TRITON)[3:5],
    }
    imgs = {}
    for name, fn in calls.items():
        v8, vs = fn(v)
        w8, ws = fn(v1)
        img, img1 = v8.view(torch.uint8), w8.view(torch.uint8)
        assert (img[:, :, Z] == 0).all() and (vs[..., Z] == 0).all(), name
        assert not torch.isnan(v8.float()).any() and torch.isfinite(vs).all(), name
        assert torch.equal(img[:, :, keep], img1[:, :, keep]) and torch.equal(vs[..., keep], ws[..., keep]), name
        imgs[name] = (img, vs)
    # the separate and the fused pre-pass stay bit-identical
    assert torch.equal(imgs["separate"][0], imgs["fused"][0]) and torch.equal(imgs["separate"][1], imgs["fused"][1])


@pytest.mark.parametrize("D", (64, 128))
def test_zero_channel_fp8_operator(D):
    import sageattention_amd as sa
    q, k, v, v1 = _qkv(D)
    for causal in (False, True):
        o, lse = sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v, is_causal=causal, return_lse=True)
        o1, lse1 = sa.sageattn_qk_int8_pv_fp8_cuda(q, k, v1, is_causal=causal, return_lse=True)
        _check_pair(o, lse, o1, lse1, D)


@pytest.mark.parametrize("D", (64, 128))
def test_zero_channel_kvlen(D):
    import sageattention_amd as sa
    q, k, v, v1 = _qkv(D, B=2)
    lens = torch.tensor([192, 100], dtype=torch.int32, device="cuda")
    o, lse = sa.sageattn_kvlen(q, k, v, lens, pv="fp8", return_lse=True)
    o1, lse1 = sa.sageattn_kvlen(q, k, v1, lens, pv="fp8", return_lse=True)
    _check_pair(o, lse, o1, lse1, D)


@pytest.mark.parametrize("D", (64, 128))
def test_zero_channel_gather_replay(D):
    """The gather schedule replayed on one GPU (3 shards of 64 rows): v_scale and v_coef of sage_kv_stats_reduce, the slot
    image, and the merged output."""
    import sageattention_amd as sa
    from test_gather_gpu import _replay
    from sageattention_amd.ring import HipGatherBackend
    q, k, v, v1 = _qkv(D)
    P, n = 3, 64
    res = _replay(sa, q, k, v, P, False, "fp8", "per_thread")
    res1 = _replay(sa, q, k, v1, P, False, "fp8", "per_thread")
    for r in range(P):
        _check_pair(res[r][0], res[r][1], res1[r][0], res1[r][1], D)
    be = HipGatherBackend("fp8", "per_thread")
    shards = [(k[:, :, r * n:(r + 1) * n], v[:, :, r * n:(r + 1) * n]) for r in range(P)]
    all_stats = torch.stack([be.stats(*s) for s in shards])
    S = be.setup(all_stats, P, *shards[0])
    assert (be.v_scale[..., Z] == 0).all() and (be.v_coef[:, :, :, Z] == 0).all() and torch.isfinite(be.v_coef).all()
    B, Hk = k.shape[:2]
    BH, kb, vb, R_ = be._layout(B, Hk, D)
    img = S.buf[0].view(n // 64, R_)[:, kb:kb + vb].reshape(n // 64, B, Hk, D, 64)
    assert (img[:, :, :, Z] == 0).all()
    assert not torch.isnan(img.contiguous().view(torch.float8_e4m3fn).float()).any()
