"""HipGatherBackend against OracleGatherBackend (tests/ring_cpu_backend.py), METHOD BY METHOD: the protocol tests run the
stand-in under gloo, the device tests replay the HIP backend end to end; here each HIP method is compared with the stand-in
method it replaces (and with the fp64 references of tests/seqpar_ref.py), on 3 shards of different content."""
import pytest
import torch

import seqpar_ref as R
from ring_cpu_backend import OracleGatherBackend
from oracle import sage_oracle as O

pytestmark = pytest.mark.gpu

BASE2 = 1.0 / 1.44269504


def _slot_parts(be, S, B, Hk, n, D, v_dtype):
    """Slot 0 of a HIP exchange buffer un-permuted from tile-major: (k8 [B,Hk,n,D] int8, ks [B,Hk,G] fp32, v) with v the
    fp8 bytes [B,Hk,D,n] (tokens of a 64-block in fp8_token_order) or the 16-bit V [B,Hk,n,D]."""
    BH, kb, vb, R_ = be._layout(B, Hk, D)
    T = n // 64
    rec = S.buf[0].cpu().view(T, R_)
    k8 = rec[:, :kb].view(torch.int8).view(T, B, Hk, 64, D).permute(1, 2, 0, 3, 4).reshape(B, Hk, n, D)
    ks = rec[:, kb + vb:kb + vb + BH * be.pt * 4].view(torch.float32).view(T, B, Hk, be.pt).permute(1, 2, 0, 3).reshape(B, Hk, T * be.pt)
    if be.pv == "fp8":
        v = rec[:, kb:kb + vb].view(T, B, Hk, D, 64).permute(1, 2, 3, 0, 4).reshape(B, Hk, D, n)
    else:
        v = rec[:, kb:kb + vb].view(v_dtype).view(T, B, Hk, 64, D).permute(1, 2, 0, 3, 4).reshape(B, Hk, n, D)
    return k8, ks, v


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("pv,gran", [("fp8", "per_thread"), ("fp16", "per_warp")])
def test_gather_backend_methods_vs_stand_in(pv, gran, D):
    from sageattention_amd.ring import HipGatherBackend
    from sageattention_amd.quant import fp8_token_order
    B, Hk, Hq, P, n, r = 1, 2, 4, 3, 128, 1
    dt = torch.float16
    g = torch.Generator().manual_seed(41 + D)
    ks = [(torch.randn(B, Hk, n, D, generator=g) * (1 + 0.5 * p) + 2 * torch.randn(1, Hk, 1, D, generator=g)).to(dt) for p in range(P)]
    # (V of unit scale and below: the absolute fp8 tolerance of test_gpu_parity.py is one e4m3 step of |v| ~ N(0,1))
    vs = [(torch.randn(B, Hk, n, D, generator=g) * (1 - 0.25 * p) + 0.3 * torch.randn(1, Hk, 1, D, generator=g)).to(dt) for p in range(P)]
    q = torch.randn(B, Hq, n, D, generator=g).to(dt)
    sm = D ** -0.5
    hip = [HipGatherBackend(pv, gran) for _ in range(P)]
    ora = [OracleGatherBackend(pv, gran) for _ in range(P)]
    c = 2 if pv == "fp8" else 1

    # -- stats: every shard against fp64
    st = [hip[p].stats(ks[p].cuda(), vs[p].cuda()) for p in range(P)]
    for p in range(P):
        assert st[p].shape == (c, B * Hk, 3, D)
        for i, x in enumerate((ks[p], vs[p])[:c]):
            R.check_stats(st[p][i].cpu(), x)
    all_h = torch.stack(st)
    all_c = all_h.cpu()

    # -- reduce: the stand-in on the same statistics gives the same bits; the mean against fp64
    _, _, ksum, kabs = (t.view(B * Hk, D) for t in R.stats_ref(torch.cat(ks, dim=2)))
    mean = ksum / (P * n)
    own_h, own_o = [], []
    for p in range(P):
        hip[p].reduce(all_h, P, P * n, ks[p].cuda(), vs[p].cuda())
        ora[p].reduce(all_c, P, P * n, ks[p], vs[p])
        assert torch.equal(R.bits(hip[p].km.cpu()), R.bits(ora[p].km))
        got = hip[p].km.cpu().double().view(B * Hk, D)
        assert ((got - mean).abs() <= R.km_tolerance(mean, got, kabs, n, D, P, P * n, dt)).all()
        if pv == "fp8":
            assert torch.equal(R.bits(hip[p].v_scale.cpu()), R.bits(ora[p].v_scale))
            assert torch.equal(R.bits(hip[p].v_coef[:, :, 1].cpu()), R.bits(O._scale_coef(O.FP8_E4M3_MAX, ora[p].amax)))
            assert (hip[p].v_coef[:, :, 0] == 0).all()
            assert torch.equal(ora[p].amax.double(), torch.cat(vs, dim=2).double().abs().amax(2))
        else:
            assert hip[p].v_scale is None and hip[p].v_coef is None
        # -- quantize: the slot holds the stand-in's bytes (it was handed the same km and amax: asserted above), tile-major
        S = hip[p].new_slots(1, B, Hk, n, D, torch.device("cuda"))
        hip[p].quantize(S, ks[p].cuda(), vs[p].cuda())
        k8, kscale, v = _slot_parts(hip[p], S, B, Hk, n, D, dt)
        w8, wscale, wv = ora[p]._quantize_parts(ks[p], vs[p])
        assert torch.equal(k8, w8) and torch.equal(R.bits(kscale), R.bits(wscale))
        if pv == "fp8":
            idx = (torch.arange(n // 64).view(-1, 1) * 64 + fp8_token_order().view(1, -1)).reshape(-1)   # position -> token
            assert torch.equal(v, wv.view(torch.uint8)[..., idx])
        else:
            assert torch.equal(R.bits(v), R.bits(wv))
        own_h.append(S.buf[0].clone())
        So = ora[p].new_slots(1, B, Hk, n, D, "cpu")
        ora[p].quantize(So, ks[p], vs[p])
        own_o.append(So.buf[0].clone())

    # -- rank r: the gathered buffer (slot p = shard of rank (r - p) mod P), the exchange replaced by copies
    Sh = hip[r].new_slots(P, B, Hk, n, D, torch.device("cuda"))
    So = ora[r].new_slots(P, B, Hk, n, D, "cpu")
    for p in range(P):
        Sh.buf[p].copy_(own_h[(r - p) % P])
        So.buf[p].copy_(own_o[(r - p) % P])

    # -- prepare_q: the same int8 queries and scales; corr = q . km within the fp32 dot-product bound of O.lse_correction
    #    (fp16 x fp16 products are exact in fp32; D - 1 additions on either side, each at most 2^-24 of sum|q km|)
    qh = hip[r].prepare_q(q.cuda(), sm, True)
    qo = ora[r].prepare_q(q, sm, True)
    assert torch.equal(qh["q8"].cpu(), qo["q8"]) and torch.equal(R.bits(qh["qs"].cpu()), R.bits(qo["qs"]))
    kmq = ora[r].km.double().repeat_interleave(Hq // Hk, dim=1).unsqueeze(2)              # [B,Hq,1,D]
    absdot = (q.double() * kmq).abs().sum(-1)
    exact = (q.double() * kmq).sum(-1)
    assert qh["corr"].shape == (B, Hq, n) and qh["corr"].dtype == torch.float32
    assert ((qh["corr"].cpu().double() - O.lse_correction(q, ora[r].km, "HND").double()).abs() <= 2 * D * R.U32 * absdot).all()
    assert ((qh["corr"].cpu().double() - exact).abs() <= D * R.U32 * absdot).all()

    # -- attend: own shard, then the two remote shards in one launch; (o, raw base-2 LSE) at the kernel-vs-oracle
    #    tolerances of test_gpu_parity.py (fp16 PV 2e-3, fp8 PV 0.06; LSE 2e-3 in natural log)
    parts_h = [hip[r].attend(qh, Sh, 0, 1, False), hip[r].attend(qh, Sh, 1, P - 1, False)]
    parts_o = [ora[r].attend(qo, So, 0, 1, False), ora[r].attend(qo, So, 1, P - 1, False)]
    for (oh, lh), (oo, lo) in zip(parts_h, parts_o):
        assert oh.dtype == dt and lh.dtype == torch.float32 and lh.shape == (B, Hq, n)
        assert (oh.cpu().float() - oo.float()).abs().max() < (2e-3 if pv == "fp16" else 0.06)
        assert ((lh.cpu() - lo) / O.LOG2E).abs().max() < 2e-3

    # -- merge: the HIP partial results merged by the kernel against the fp64 merge of the same partial results
    o, lse = hip[r].merge(parts_h, qh, True)
    flat_o = [t[0].cpu().reshape(-1, D) for t in parts_h]
    flat_l = [t[1].cpu().reshape(-1) for t in parts_h]
    ref = R.merge_ref(flat_o, flat_l, BASE2, qh["corr"].cpu().reshape(-1), sm)
    R.check_merge(o.cpu().reshape(-1, D), lse.cpu().reshape(-1), ref, dt)
    # ... and the stand-in's merge of ITS partial results, at the attention tolerances
    oo, lo = ora[r].merge(parts_o, qo, True)
    assert (o.cpu().float() - oo.float()).abs().max() < (2e-3 if pv == "fp16" else 0.06)
    assert (lse.cpu() - lo).abs().max() < 2e-3
    # -- want_lse = False: no correction is computed, no LSE comes back, o is the same
    qn = hip[r].prepare_q(q.cuda(), sm, False)
    assert qn["corr"] is None and torch.equal(qn["q8"], qh["q8"])
    o2, none = hip[r].merge(parts_h, qn, False)
    assert none is None and torch.equal(R.bits(o2.cpu()), R.bits(o.cpu()))
    # a single part: merge is sage_finish_lse on the raw LSE
    o1, l1 = hip[r].merge(parts_h[:1], qh, True)
    assert o1 is parts_h[0][0]
    assert torch.equal(R.bits(l1.cpu().reshape(-1)), R.bits(R.finish_lse_ref(flat_l[0], qh["corr"].cpu().reshape(-1), sm)))
