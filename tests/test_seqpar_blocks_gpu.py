"""The sequence-parallel building blocks, kernel by kernel, against the plain fp64 references of tests/seqpar_ref.py:
sage_seq_stats, sage_kv_stats_reduce, sage_merge_attn_states_multi(_ex), HipRingBackend.merge_all, the in-place two-way
sage_merge_attn_states and sage_finish_lse.  The end-to-end tests (test_gather_gpu.py, test_gpu_parity.py) absorb an error
in any of these by construction: the smoothing mean cancels in the softmax, a merge weight off by 1e-3 sits inside the
operator's tolerance.  Bounds: exact where the arithmetic is exact, otherwise derived in seqpar_ref.py (one measured
constant, EPS_EXP)."""
import ctypes

import numpy as np
import pytest
import torch

import seqpar_ref as R
from ring_cpu_backend import OracleGatherBackend
from oracle import sage_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
IDS = ("fp16", "bf16")
BASE2 = 1.0 / 1.44269504


def _L():
    from sageattention_amd import _lib as L
    return L


# ----------------------------------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------------------------------

def _seq_stats(x):
    """sage_seq_stats of an HND tensor / view -> fp32 [B*H,3,D] (output poisoned first)."""
    L = _L()
    B, H, N, D = x.shape
    out = torch.full((B * H, 3, D), float("nan"), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(1, L.lib().sage_seq_stats_workspace_bytes(B, H, N, D) // 4), dtype=torch.float32, device=x.device)
    L.check(L.lib().sage_seq_stats(L.desc(x, "HND"), L.dtype_code(x.dtype), B, H, N, D, out.data_ptr(), ws.data_ptr(),
                                   L.stream_ptr(x.device)), "sage_seq_stats")
    return out


def _stats_data(B, H, N, D, dt, seed, scale=1.0):
    """randn plus per-channel offsets of -3 / 0 / +3: some channels are one-signed."""
    g = torch.Generator().manual_seed(seed)
    off = (torch.randint(0, 3, (1, H, 1, D), generator=g) - 1) * 3.0
    return (torch.randn(B, H, N, D, generator=g) * scale + off).to(dt)


@pytest.mark.parametrize("N", (64, 200, 256, 2048, 2304, 4160))
@pytest.mark.parametrize("layout", ("HND", "NHD"))
@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_seq_stats_vs_fp64(dt, D, layout, N):
    """N: a partial chunk (64, 200 -- and 200 % 16 != 0), exactly one chunk, 8 chunks, 9 (second trip of the 8-in-flight
    loop of seq_stats_final_kernel with a tail of one) and 17."""
    B, H = 2, 3
    x = _stats_data(B, H, N, D, dt, seed=N + D)
    xd = x.cuda() if layout == "HND" else x.transpose(1, 2).contiguous().cuda().transpose(1, 2)   # HND view of NHD memory
    assert xd.is_contiguous() == (layout == "HND")
    st = _seq_stats(xd).cpu()
    R.check_stats(st, x)
    assert torch.equal(R.bits(_seq_stats(xd).cpu()), R.bits(st))                                     # deterministic


# ----------------------------------------------------------------------------------------------------------------------
# reduce
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_v", (False, True), ids=("k", "kv"))
@pytest.mark.parametrize("parts", (1, 3, 8))
@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_kv_stats_reduce(dt, D, parts, with_v):
    L = _L()
    B, Hk, n = 1, 2, 192
    BH, c = B * Hk, 2 if with_v else 1
    ks = [_stats_data(B, Hk, n, D, dt, seed=10 * p + D) for p in range(parts)]
    vs = [_stats_data(B, Hk, n, D, dt, seed=10 * p + D + 5, scale=p + 1.0) for p in range(parts)]
    stride = c * BH * 3 * D + 40                                   # larger than minimal; the gaps hold NaN and are not read
    buf = torch.full((parts, stride), float("nan"), dtype=torch.float32, device="cuda")
    for p in range(parts):
        buf[p, :BH * 3 * D] = _seq_stats(ks[p].cuda()).reshape(-1)
        if with_v:
            buf[p, BH * 3 * D:2 * BH * 3 * D] = _seq_stats(vs[p].cuda()).reshape(-1)
    n_total = parts * n
    km = torch.full((BH, D), float("nan"), dtype=dt, device="cuda")
    v_scale = torch.full((BH, D), float("nan"), dtype=torch.float32, device="cuda") if with_v else None
    v_coef = torch.full((BH, 2, D), float("nan"), dtype=torch.float32, device="cuda") if with_v else None
    L.check(L.lib().sage_kv_stats_reduce(buf.data_ptr(), buf[0, BH * 3 * D:].data_ptr() if with_v else None, parts, stride, BH,
                                         D, n_total, L.dtype_code(dt), 448.0, km.data_ptr(), L.ptr(v_scale), L.ptr(v_coef),
                                         L.stream_ptr(buf.device)), "sage_kv_stats_reduce")
    torch.cuda.synchronize()
    all_stats = buf[:, :c * BH * 3 * D].cpu().view(parts, c, BH, 3, D)
    assert torch.isfinite(all_stats).all()
    # the stand-in on the GPU's own statistics: the same bits
    be = OracleGatherBackend("fp8" if with_v else "fp16", "per_thread")
    be.reduce(all_stats, parts, n_total, ks[0], vs[0])
    assert torch.equal(R.bits(km.cpu()), R.bits(be.km.view(BH, D)))
    if with_v:
        assert torch.equal(R.bits(v_scale.cpu()), R.bits(be.v_scale.view(BH, D)))
        assert torch.equal(R.bits(v_coef[:, 1].cpu()), R.bits(O._scale_coef(O.FP8_E4M3_MAX, be.amax).view(BH, D)))
        assert (v_coef[:, 0] == 0).all()
        ref = R.reduce_ref(all_stats, n_total, dt)
        assert torch.equal(R.bits(v_scale.cpu()), R.bits(ref.v_scale)) and torch.equal(R.bits(v_coef[:, 1].cpu()), R.bits(ref.v_coef))
        true_amax = torch.cat(vs, dim=2).double().abs().amax(2).view(BH, D)
        assert torch.equal(ref.amax.double(), true_amax)
    # the whole-sequence mean against fp64
    _, _, sm, sa = (t.view(BH, D) for t in R.stats_ref(torch.cat(ks, dim=2)))
    mean = sm / n_total
    got = km.cpu().double()
    err = (got - mean).abs()
    tol = R.km_tolerance(mean, got, sa, n, D, parts, n_total, dt)
    assert (err <= tol).all(), (err / tol).max().item()


# ----------------------------------------------------------------------------------------------------------------------
# multi-way merge
# ----------------------------------------------------------------------------------------------------------------------

def _merge_multi(os_, ls, dt, D, ex=None, want_lse=True):
    """sage_merge_attn_states_multi (ex None) or _multi_ex (ex = (in_mult, corr or None, corr_mult)) on CPU inputs.
    -> (o, lse) on the CPU.  want_lse False: lse_out = NULL, and `lse` is the poisoned buffer that stands right behind o in the
    same allocation, where lse_out would be."""
    L = _L()
    count, rows = len(os_), ls[0].numel()
    od, ld = [t.cuda() for t in os_], [t.cuda() for t in ls]
    blob = torch.full((rows * D * 2 + rows * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    o = blob[:rows * D * 2].view(dt).view(rows, D)
    lse = blob[rows * D * 2:].view(torch.float32)
    op = (ctypes.c_void_p * count)(*[t.data_ptr() for t in od])
    lp = (ctypes.c_void_p * count)(*[t.data_ptr() for t in ld])
    st = L.stream_ptr(blob.device)
    lse_ptr = lse.data_ptr() if want_lse else None
    if ex is None:
        s = L.lib().sage_merge_attn_states_multi(op, lp, count, L.dtype_code(dt), o.data_ptr(), lse_ptr, rows, D, st)
    else:
        im, corr, cm = ex
        cd = None if corr is None else corr.cuda()
        s = L.lib().sage_merge_attn_states_multi_ex(op, lp, count, L.dtype_code(dt), o.data_ptr(), lse_ptr, rows, D, float(im),
                                                    L.ptr(cd), float(cm), st)
    L.check(s, "sage_merge_attn_states_multi")
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu()


def check_merge_exact(c, o, lse, count, im=1.0, has_corr=False):
    """The assertions without tolerance, per kind of the menu."""
    kinds = c.kind
    for ki, name in enumerate(R.KINDS):
        m = kinds == ki
        if not m.any():
            continue
        if name == "f" or (count == 1 and name.startswith("e_")):      # nothing attended: (0, -inf), with a finite corr too
            assert (o[m].float() == 0).all()
            assert lse is None or torch.isneginf(lse[m]).all()
        elif name.startswith("c_") or count == 1:                      # the dominant (or only) block comes back bit for bit
            s = max(R.kind_slot(name, count), 0)
            assert torch.equal(R.bits(o[m]), R.bits(c.os[s][m])), name
            if lse is not None and not has_corr:                       # ... and lse is its LSE (scaled by ONE fp32 product)
                want = torch.from_numpy(c.lses[s][m].numpy() * np.float32(im))
                assert torch.equal(R.bits(lse[m]), R.bits(want)), name
        elif name == "b" and count in (2, 4, 8, 16):                   # count * o / count: every step exact
            assert torch.equal(R.bits(o[m]), R.bits(c.os[0][m]))
        if name.startswith("e_"):
            assert not torch.isnan(o[m].float()).any()


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("count", (1, 2, 3, 4, 5, 8, 9, 15, 16))
def test_merge_multi_vs_fp64(count, dt, D):
    """Counts that fill the 2 / 4 / 8 / 16-slot instances and counts below their capacity (3, 5, 9, 15); 1, 31, 33 and 1000
    rows (a block of 256 threads partly filled, the last block of the grid); the whole menu of seqpar_ref.merge_cases."""
    sm = D ** -0.5
    for rows in (1, 31, 33, 1000):
        g = torch.Generator().manual_seed(rows)
        corr = torch.randn(rows, generator=g) * 4
        variants = [("multi", 1.0, None, 0.0), ("ex", BASE2, corr, sm), ("ex", BASE2, None, 0.0)]
        for which, im, cr, cm in variants:
            c = R.merge_cases(count, rows, D, dt, in_mult=im)
            ex = None if which == "multi" else (im, cr, cm)
            ref = R.merge_ref(c.os, c.lses, im, cr, cm)
            o, lse = _merge_multi(c.os, c.lses, dt, D, ex)
            R.check_merge(o, lse, ref, dt)
            check_merge_exact(c, o, lse, count, im, cr is not None)
            o2, lse2 = _merge_multi(c.os, c.lses, dt, D, ex)                       # two launches: the same bits
            assert torch.equal(R.bits(o2), R.bits(o)) and torch.equal(R.bits(lse2), R.bits(lse))
            if which == "ex":                                                      # lse_out = NULL: o unchanged, nothing written
                o3, guard = _merge_multi(c.os, c.lses, dt, D, ex, want_lse=False)
                assert torch.equal(R.bits(o3), R.bits(o))
                assert (guard.view(torch.uint8) == 0xA5).all()


def test_merge_multi_rejects_17_blocks():
    L = _L()
    t = torch.zeros(8, 64, dtype=torch.float16, device="cuda")
    l = torch.zeros(8, dtype=torch.float32, device="cuda")
    op = (ctypes.c_void_p * 17)(*[t.data_ptr()] * 17)
    lp = (ctypes.c_void_p * 17)(*[l.data_ptr()] * 17)
    o = torch.empty_like(t)
    assert L.lib().sage_merge_attn_states_multi(op, lp, 17, L.SAGE_F16, o.data_ptr(), l.data_ptr(), 8, 64, None) == -1
    assert L.lib().sage_merge_attn_states_multi_ex(op, lp, 17, L.SAGE_F16, o.data_ptr(), l.data_ptr(), 8, 64, 1.0, None, 0.0,
                                                   None) == -1


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_ring_merge_all_18_blocks(dt):
    """HipRingBackend.merge_all regroups 18 blocks as 16 + (result, 2 rest): one more rounding of o to the storage type (at
    most half an ulp of w * o <= 2^-(mant+1) * sum_i w_i|o_i|) and a second pass of the fp32 errors."""
    from sageattention_amd.ring import HipRingBackend
    count, B, H, M, D = 18, 1, 2, 33, 64
    c = R.merge_cases(count, B * H * M, D, dt)
    blocks = [(o.view(B, H, M, D).cuda(), l.view(B, H, M).cuda()) for o, l in zip(c.os, c.lses)]
    o, lse = HipRingBackend().merge_all(blocks)
    assert o.shape == (B, H, M, D) and lse.shape == (B, H, M) and o.dtype == dt
    ref = R.merge_ref(c.os, c.lses)
    mant = 10 if dt == torch.float16 else 7
    R.check_merge(o.cpu().view(-1, D), lse.cpu().view(-1), ref, dt, o_extra=2.0 ** -(mant + 1) * ref.wabs, passes=2)
    f = c.kind == R.KINDS.index("f")
    assert (o.cpu().view(-1, D)[f] == 0).all() and torch.isneginf(lse.cpu().view(-1)[f]).all()


# ----------------------------------------------------------------------------------------------------------------------
# in-place two-way merge
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("count", (1, 2, 5))
def test_two_way_merge_fold_vs_fp64(count, dt, D):
    """sage_merge_attn_states folded over the blocks into an fp32 accumulator that starts EMPTY -- lse_acc = -inf, o_acc
    holding NaN and Inf, the natural start of a ring (a torch.empty accumulator) -- with empty blocks (lse = -inf, NaN o)
    among them.  The result is finite and is the merge of the non-empty blocks; both sides empty gives (0, -inf).  The bound
    is the multi-way one without the output ulp (the accumulator is fp32)."""
    L = _L()
    rows = 333
    c = R.merge_cases(count, rows, D, dt)
    acc = torch.full((rows, D), float("nan"), dtype=torch.float32, device="cuda")
    acc[1::3] = float("inf")
    acc[2::3] = float("-inf")
    lse = torch.full((rows,), float("-inf"), dtype=torch.float32, device="cuda")
    for o_b, l_b in zip(c.os, c.lses):
        ob, lb = o_b.cuda(), l_b.cuda()
        L.check(L.lib().sage_merge_attn_states(acc.data_ptr(), lse.data_ptr(), ob.data_ptr(), L.dtype_code(dt), lb.data_ptr(),
                                               rows, D, L.stream_ptr(acc.device)), "sage_merge_attn_states")
    torch.cuda.synchronize()
    acc, lse = acc.cpu(), lse.cpu()
    ref = R.merge_ref(c.os, c.lses)
    o_tol, l_tol = R.merge_tolerances(ref, None)
    assert torch.isfinite(acc).all() and not torch.isnan(lse).any()
    assert torch.equal(torch.isneginf(lse), torch.isneginf(ref.lse))
    empty = torch.isneginf(ref.lse)
    assert empty.any() and (acc[empty] == 0).all()
    fin = ~empty
    e = (lse.double() - ref.lse).abs()
    assert (e[fin] <= l_tol[fin]).all(), (e[fin] / l_tol[fin]).max().item()
    e = (acc.double() - ref.o).abs()
    assert (e <= o_tol).all(), (e / o_tol.clamp(min=1e-300)).max().item()


# ----------------------------------------------------------------------------------------------------------------------
# sage_finish_lse
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_corr", (False, True))
@pytest.mark.parametrize("D", (128, 64))
@pytest.mark.parametrize("n", (1, 255, 256, 257))
def test_finish_lse_bit_identical(n, D, with_corr):
    L = _L()
    sm = D ** -0.5
    g = torch.Generator().manual_seed(n)
    lse2 = torch.randn(n, generator=g) * 20
    lse2[::5] = float("-inf")
    corr = torch.randn(n, generator=g) * 5 if with_corr else None
    l2, cd = lse2.cuda(), None if corr is None else corr.cuda()
    blob = torch.full((n + 64,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(L.lib().sage_finish_lse(l2.data_ptr(), L.ptr(cd), float(sm), blob.data_ptr(), n, L.stream_ptr(l2.device)),
            "sage_finish_lse")
    torch.cuda.synchronize()
    out = blob.cpu()
    assert torch.isnan(out[n:]).all()                                  # nothing past n
    want = R.finish_lse_ref(lse2, corr, sm)
    assert torch.equal(R.bits(out[:n]), R.bits(want))
    assert torch.isneginf(out[:n][::5]).all()
