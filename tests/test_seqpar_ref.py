"""The fp64 references of tests/seqpar_ref.py and the CPU stand-ins of tests/ring_cpu_backend.py (plus the oracle's two-way
merge) check each other on the case tables the GPU tests use -- no GPU needed.  Also here: the menu of merge_cases holds
what it promises, and the FP8 V quantizer of the oracle and of the stand-in is defined on a channel that is zero over the
whole sequence (all-0x00 image, v_scale 0, no NaN)."""
import numpy as np
import pytest
import torch

import seqpar_ref as R
from oracle import sage_oracle as O
from ring_cpu_backend import OracleGatherBackend, OracleRingBackend

COUNTS = (1, 2, 3, 4, 5, 8, 9, 15, 16)
DTYPES = (torch.float16, torch.bfloat16)
BASE2 = 1.0 / 1.44269504


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("count", COUNTS)
def test_merge_menu(count, dt):
    """Every (count, dtype) table of the GPU tests with at least len(KINDS) rows holds every kind, and each kind is what
    the menu says (on the scaled LSEs l * in_mult)."""
    for rows in (31, 33, 1000):
        for im in (1.0, BASE2):
            c = R.merge_cases(count, rows, 64, dt, in_mult=im)
            assert sorted(set(c.kind.tolist())) == list(range(len(R.KINDS)))
            l = torch.stack(c.lses) * float(np.float32(im))          # as the kernel scales them (one fp32 product)
            o = torch.stack(c.os)
            for ki, name in enumerate(R.KINDS):
                m = c.kind == ki
                lk, ok = l[:, m], o[:, m]
                if name in ("a", "b", "d_plus", "d_minus") or name.startswith("c_"):
                    assert torch.isfinite(lk).all() and torch.isfinite(ok.float()).all()
                if name == "b":
                    assert (lk == lk[0]).all() and (ok == ok[0]).all()
                elif name.startswith("c_"):
                    s = R.kind_slot(name, count)
                    assert (c.slot[m] == s).all()
                    rest = lk.clone()
                    rest[s] = float("-inf")
                    if count > 1:
                        assert (lk[s] - rest.amax(0) >= R.DOMINANT_GAP).all()
                        assert np.exp(np.float32(-R.DOMINANT_GAP)) == 0.0       # fp32 exp(-110) is 0
                elif name.startswith("d_"):
                    assert (lk.abs() > 2.9e4).all() and ((lk > 0) == (name == "d_plus")).all()
                elif name.startswith("e_"):
                    s = R.kind_slot(name, count)
                    assert torch.isneginf(lk[s]).all() and not torch.isfinite(ok[s].float()).any()
                    assert torch.isnan(ok[s].float()).any() and torch.isposinf(ok[s].float()).any() and torch.isneginf(ok[s].float()).any()
                    others = [i for i in range(count) if i != s]
                    assert torch.isfinite(lk[others]).all()
                elif name == "f":
                    assert torch.isneginf(lk).all()


def _check_merge(o, lse, ref, dt, roundings=1):
    o_tol, l_tol = R.merge_tolerances(ref, dt, roundings)
    assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
    assert torch.equal(torch.isneginf(lse), torch.isneginf(ref.lse))
    fin = torch.isfinite(ref.lse)
    assert ((lse.double() - ref.lse).abs()[fin] <= l_tol[fin]).all()
    assert ((o.double() - ref.o).abs() <= o_tol).all()


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("count", COUNTS)
def test_merge_ref_vs_ring_stand_in(count, dt):
    """OracleRingBackend.merge_all (fp32 torch) against merge_ref (fp64) at the bounds the HIP kernel is held to."""
    c = R.merge_cases(count, 200, 64, dt)
    ref = R.merge_ref(c.os, c.lses)
    o, lse = OracleRingBackend().merge_all(list(zip(c.os, c.lses)))
    assert o.dtype == dt
    _check_merge(o, lse, ref, dt)
    f = c.kind == R.KINDS.index("f")
    assert (o[f] == 0).all() and torch.isneginf(lse[f]).all()


@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("count", (2, 3, 5, 16))
def test_merge_ref_vs_gather_stand_in(count, dt):
    """OracleGatherBackend.merge: base-2 LSEs, one correction (q.km) * sm_scale added after the merge."""
    D = 128
    c = R.merge_cases(count, 200, D, dt, in_mult=BASE2)
    corr = torch.randn(200, generator=torch.Generator().manual_seed(count)) * 4
    sm = D ** -0.5
    ref = R.merge_ref(c.os, c.lses, BASE2, corr, sm)
    o, lse = OracleGatherBackend().merge(list(zip(c.os, c.lses)), {"corr": corr, "sm_scale": sm}, True)
    _check_merge(o, lse, ref, dt)
    o2, none = OracleGatherBackend().merge(list(zip(c.os, c.lses)), {"corr": None, "sm_scale": sm}, False)
    assert none is None and torch.equal(o2.view(torch.int16), o.view(torch.int16))


def test_merge_ref_vs_oracle_two_way():
    """O.merge_attn_states folded over the blocks, from an empty accumulator whose o is poisoned, against merge_ref."""
    for count in (1, 2, 5):
        c = R.merge_cases(count, 200, 64, torch.float16)
        ref = R.merge_ref(c.os, c.lses)
        acc = torch.full((200, 64), float("nan"))
        lse = torch.full((200,), float("-inf"))
        for o_b, l_b in zip(c.os, c.lses):
            acc, lse = O.merge_attn_states(acc, lse, o_b, l_b)
        f = c.kind == R.KINDS.index("f")
        # (the oracle's logaddexp(-inf, -inf) is -inf; its weights exp(-inf - -inf) are NaN there and masked to 0)
        assert torch.isneginf(lse[f]).all() and (acc[f] == 0).all()
        o_tol, l_tol = R.merge_tolerances(ref, None)
        fin = torch.isfinite(ref.lse)
        assert not torch.isnan(acc).any()
        assert ((lse.double() - ref.lse).abs()[fin] <= count * l_tol[fin]).all()
        assert ((acc.double() - ref.o).abs() <= count * o_tol + 1e-30).all()


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_stats_and_reduce_ref_vs_gather_stand_in(dt, D):
    """stats_ref / reduce_ref against OracleGatherBackend.stats / reduce over 3 shards of different content."""
    g = torch.Generator().manual_seed(D)
    B, Hk, n, P = 1, 2, 192, 3
    off = (torch.randint(0, 3, (1, Hk, 1, D), generator=g) - 1) * 3.0
    ks = [(torch.randn(B, Hk, n, D, generator=g) + off).to(dt) for _ in range(P)]
    vs = [(torch.randn(B, Hk, n, D, generator=g) * (p + 1) + off).to(dt) for p in range(P)]
    be = OracleGatherBackend("fp8", "per_thread")
    sts = []
    for k, v in zip(ks, vs):
        st = be.stats(k, v)
        for i, x in enumerate((k, v)):
            mx, mn, sm, sa = R.stats_ref(x)
            assert torch.equal(st[i, :, 0].double(), mx.view(B * Hk, D)) and torch.equal(st[i, :, 1].double(), mn.view(B * Hk, D))
            # torch's fp32 sum is a cascade whose depth is below the kernel's addition count: the kernel's bound holds for it
            assert ((st[i, :, 2].double() - sm.view(B * Hk, D)).abs() <= R.sum_bound(sa, n, D).view(B * Hk, D)).all()
        sts.append(st)
    all_stats = torch.stack(sts)
    be.reduce(all_stats, P, P * n, ks[0], vs[0])
    ref = R.reduce_ref(all_stats, P * n, dt)
    assert torch.equal(be.amax.view(-1, D), ref.amax)
    assert torch.equal(be.v_scale.view(-1, D), ref.v_scale)
    assert torch.equal(O._scale_coef(O.FP8_E4M3_MAX, be.amax).view(-1, D), ref.v_coef)
    # km: the stand-in sums the shard sums in fp32 (P additions) and divides once; then one rounding to the storage type
    sum_abs = all_stats[:, 0, :, 2, :].double().abs().sum(0)
    tol = 0.5 * R.ulp(ref.mean, dt) + (P + 1) * R.U32 * sum_abs / (P * n) * (1 + 2.0 ** -8)
    assert ((be.km.double().view(-1, D) - ref.mean).abs() <= tol).all()
    # and against the true mean of the concatenated sequence
    _, _, sm, sa = R.stats_ref(torch.cat(ks, dim=2))
    true_mean = sm.view(-1, D) / (P * n)
    tol = 0.5 * R.ulp(true_mean, dt) * (1 + 2.0 ** -8) + R.sum_bound(sa, n, D, P).view(-1, D) / (P * n)
    assert ((be.km.double().view(-1, D) - true_mean).abs() <= tol).all()


def test_finish_lse_ref_is_the_torch_expression():
    """finish_lse_ref (numpy float32) is bit for bit `lse2 / 1.44269504 + corr * sm_scale` as torch evaluates it on fp32
    tensors (core.py:651), -inf staying -inf."""
    g = torch.Generator().manual_seed(3)
    lse2 = torch.randn(4097, generator=g) * 20
    lse2[::97] = float("-inf")
    corr = torch.randn(4097, generator=g) * 5
    for sm in (128 ** -0.5, 64 ** -0.5):
        assert torch.equal(R.finish_lse_ref(lse2, corr, sm), lse2 / 1.44269504 + corr * sm)
        assert torch.equal(R.finish_lse_ref(lse2, None, sm), lse2 / 1.44269504)
    assert torch.isneginf(R.finish_lse_ref(lse2, corr, 0.125)[::97]).all()


@pytest.mark.parametrize("D", (64, 128))
def test_zero_v_channel_is_defined_in_oracle_and_stand_in(D):
    """A V channel that is zero over the whole sequence: all-0x00 image row, v_scale == 0, no NaN anywhere -- in
    O.per_channel_fp8 and in OracleGatherBackend._quantize_parts.  The other channels are those of the same V with the dead
    channel set to 1.0 (the scale is per channel)."""
    g = torch.Generator().manual_seed(5)
    B, H, N, z = 1, 2, 192, 5
    v = torch.randn(B, H, N, D, generator=g).half()
    v[..., z] = 0
    v1 = v.clone()
    v1[..., z] = 1.0
    for smooth in (False, True):
        v8, vs, _ = O.per_channel_fp8(v, "HND", smooth_v=smooth)
        img = v8.view(torch.uint8)
        assert (img[:, :, z] == 0).all() and (vs[..., z] == 0).all()
        assert not torch.isnan(v8.float()).any() and torch.isfinite(vs).all()
        w8, ws, _ = O.per_channel_fp8(v1, "HND", smooth_v=smooth)
        keep = [d for d in range(D) if d != z]
        assert torch.equal(img[:, :, keep], w8.view(torch.uint8)[:, :, keep]) and torch.equal(vs[..., keep], ws[..., keep])
    be = OracleGatherBackend("fp8", "per_thread")
    k = torch.randn(B, H, N, D, generator=g).half()
    be.reduce(be.stats(k, v).unsqueeze(0), 1, N, k, v)
    assert (be.v_scale[..., z] == 0).all() and torch.isfinite(be.v_scale).all()
    _, _, img = be._quantize_parts(k, v)
    assert (img.view(torch.uint8)[:, :, z] == 0).all() and not torch.isnan(img.float()).any()
    assert torch.equal(img.view(torch.uint8), O.per_channel_fp8(v, "HND", smooth_v=False)[0].view(torch.uint8))
