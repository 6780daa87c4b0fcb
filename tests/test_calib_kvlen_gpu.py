"""Calibration with per-batch key lengths on the GPU: sageattn_tile_mass_kvlen, plan_recall_kvlen and sparge_tune_kvlen
(the rule: include/sageattn_hip.h, calibration with per-batch key lengths).

The reference for batch b is the existing function on the slice -- ``sageattn_tile_mass`` on ``q[b:b+1]`` and the first len_b
keys, ``plan_recall`` on the map and the mass cut to ceil(len_b / 64) columns, on the same GPU -- and for the tuner the whole
grid evaluated through the public ``sparge_plan(kv_lens=)`` + ``plan_recall_kvlen`` with the reductions its docstring states.
Every comparison is ``torch.equal`` unless said otherwise: the rule admits no tolerance.  In every case the K rows >= len_b
hold NaN, so anything that reads them -- a statistic of the pre-pass or of the pooling, a staged row that is not masked --
shows."""
import functools

import pytest
import torch

import blocksparse_util as BU
import calib_util as C
import pvskip_util as PU
import sparge_util as SU
import test_calib_gpu as G

pytestmark = pytest.mark.gpu

HQ, HK, M, N = 4, 2, 200, 320
LENS = [320, 257, 256, 65, 1, 0]   # full; one row into the last tile; whole tiles; one row into tile 1; one key; none
INF = float("inf")


@pytest.fixture(scope="module")
def sa():
    import sageattention_amd
    return sageattention_amd


def _lens(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


def _clamped(lens, n):
    return [min(max(int(x), 0), n) for x in lens]


def _ntk(n):
    return (n + 63) // 64


def _make(B, D, dtype=torch.float16, seed=0, layout="HND"):
    """seeded q [B,HQ,M,D], k [B,HK,N,D] on the GPU; k carries a per-channel offset, so that the smoothing mean matters"""
    g = torch.Generator().manual_seed(1000 * D + seed)
    q = torch.randn(B, HQ, M, D, generator=g)
    k = torch.randn(B, HK, N, D, generator=g) + 2.0 * torch.randn(B, HK, 1, D, generator=g)
    q, k = q.to(dtype).cuda(), k.to(dtype).cuda()
    if layout == "NHD":
        q, k = q.transpose(1, 2).contiguous(), k.transpose(1, 2).contiguous()
    return q, k


def _poison(k, eff, layout="HND"):
    """NaN into the K rows >= len_b"""
    for b, n in enumerate(eff):
        if layout == "HND":
            k[b, :, n:] = float("nan")
        else:
            k[b, n:] = float("nan")
    return k


def _keys(k, b, n, layout="HND"):
    return k[b:b + 1, :, :n] if layout == "HND" else k[b:b + 1, :n]


def _check_mass_against_the_slices(sa, q, k, lens, gran, layout="HND"):
    """the assertions of case 1 for one set of inputs; ``lens`` may lie outside [0, N]"""
    eff = _clamped(lens, N)
    _poison(k, eff, layout)
    mass = sa.sageattn_tile_mass_kvlen(q, k, _lens(lens), tensor_layout=layout, qk_quant_gran=gran)
    torch.cuda.synchronize()
    assert mass.dtype == torch.float32 and tuple(mass.shape) == (len(lens), HQ, (M + 127) // 128, _ntk(N))
    D = q.shape[-1]
    for b, n in enumerate(eff):
        nb = _ntk(n)
        assert torch.equal(mass[b, :, :, nb:], torch.zeros_like(mass[b, :, :, nb:])), f"batch {b} (len {n}): columns >= ntk_b"
        if n == 0:
            continue
        ref = sa.sageattn_tile_mass(q[b:b + 1], _keys(k, b, n, layout), tensor_layout=layout, qk_quant_gran=gran)
        assert torch.isfinite(ref).all(), "the reference itself"
        assert torch.equal(mass[b:b + 1, :, :, :nb], ref), (f"batch {b} (len {n}): differs in "
                                                            f"{int((mass[b:b + 1, :, :, :nb] != ref).sum())} of {ref.numel()} entries")
        # rows sum to 1 within the tolerance tests/test_calib_gpu.py derives, for the logits of this slice (head_dim padded
        # with zeros as the operator pads it: the quantization does not see them)
        qc, kc = q[b:b + 1].cpu(), _keys(k, b, n, layout).cpu()
        if layout == "NHD":
            qc, kc = qc.transpose(1, 2), kc.transpose(1, 2)
        pad = (128 if D > 64 else 64) - D
        logits = PU.scaled_logits(torch.nn.functional.pad(qc, (0, pad)), torch.nn.functional.pad(kc, (0, pad)), gran,
                                  sm_scale=D ** -0.5)
        eps = G.eps_for(logits, n)
        dev = (mass[b].double().sum(-1) - 1).abs().max()
        print(f"tile mass kvlen D={D} {gran} {q.dtype} {layout} batch {b} len {n}: eps = {eps:.3e}, max |row sum - 1| = {float(dev):.3e}")
        assert float(dev) <= eps, (b, n, float(dev), eps)
    return mass


# ---- 1. tile mass on slices ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
@pytest.mark.parametrize("D", [64, 128])
def test_tile_mass_against_the_slices(sa, D, gran, dtype):
    """N = 320 (five tiles), M = 200 (two q-blocks, the second ragged: one wave partly and one wholly beyond M), lengths that
    end on and off a tile edge, one key, no key"""
    q, k = _make(len(LENS), D, dtype)
    mass = _check_mass_against_the_slices(sa, q, k, LENS, gran)
    assert torch.equal(mass[5], torch.zeros_like(mass[5])), "the batch without keys"


def test_tile_mass_nhd_head_dim_72(sa):
    q, k = _make(len(LENS), 72, seed=2, layout="NHD")
    _check_mass_against_the_slices(sa, q, k, LENS, "per_thread", layout="NHD")


# ---- 2. / 3. clamping, full lengths ----------------------------------------------------------------------------------------
def test_lengths_outside_the_range_are_clamped(sa):
    q, k = _make(4, 64, seed=3)
    mass = _check_mass_against_the_slices(sa, q, k, [-5, N + 100, 1 << 30, 100], "per_thread")
    assert torch.equal(mass[0], torch.zeros_like(mass[0]))
    rec, kept = sa.plan_recall_kvlen(torch.ones(4, HQ, 2, 5, dtype=torch.bool, device="cuda"), mass,
                                     _lens([-5, N + 100, 1 << 30, 100]))
    assert kept[:, 0, 0].tolist() == [0, 5, 5, 2]


@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
@pytest.mark.parametrize("D", [64, 128])
def test_full_lengths_give_the_mass_without_lengths(sa, D, gran):
    q, k = _make(3, D, seed=4)
    full = torch.full((3,), N, dtype=torch.int32, device="cuda")
    want = sa.sageattn_tile_mass(q, k, qk_quant_gran=gran)
    assert torch.equal(sa.sageattn_tile_mass_kvlen(q, k, full, qk_quant_gran=gran), want)
    bm = BU.make_map(3, HQ, M, N, 0.5, 21).cuda()
    a, b = sa.plan_recall_kvlen(bm, want, full), sa.plan_recall(bm, want)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. poisoned operands --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
@pytest.mark.parametrize("D", [64, 128])
def test_nothing_beyond_the_length_is_read_and_every_entry_is_written(sa, D, gran):
    """the raw entry point on the operands of k_smooth_quant_kvlen, then again with 127 in the k8 rows >= len_b, NaN in the
    scales of the tiles >= ntk_b and NaN in the output buffer: the same bits"""
    from sageattention_amd import _lib as L, core
    from sageattention_amd.quant import k_smooth_quant_kvlen
    B = len(LENS)
    q, k = _make(B, D, seed=5)
    _poison(k, LENS)
    kv_lens = _lens(LENS)
    k8, ks, km = k_smooth_quant_kvlen(k, kv_lens, "HND", *core._k_pairing(gran))
    q8, qs, _ = core._quant_q(q, km, "HND", gran, D ** -0.5, 32, False, HQ, HK)
    per_tile = 4 if gran == "per_thread" else 1
    assert tuple(ks.shape) == (B, HK, _ntk(N) * per_tile)

    def run(k8, ks, fill):
        mass = torch.full((B, HQ, 2, _ntk(N)), fill, dtype=torch.float32, device="cuda")
        st = L.lib().sage_attn_tile_mass_kvlen(L.desc(q8, "HND"), L.desc(k8, "HND"), qs.data_ptr(), ks.data_ptr(), B, HQ, HK, M,
                                               N, D, core._GRAN_CODE[gran], 128, 32, D ** -0.5, 0, mass.data_ptr(),
                                               kv_lens.data_ptr(), L.stream_ptr(q.device))
        assert st == 0
        torch.cuda.synchronize()
        return mass
    clean = run(k8, ks, 0.0)
    assert torch.equal(clean, sa.sageattn_tile_mass_kvlen(q, k, kv_lens, qk_quant_gran=gran))  # the public function is this call
    k8p, ksp = k8.clone(), ks.clone()
    for b, n in enumerate(LENS):
        k8p[b, :, n:] = 127
        ksp[b, :, _ntk(n) * per_tile:] = float("nan")
    got = run(k8p, ksp, float("nan"))
    assert not torch.isnan(got).any(), "every entry is written, and no NaN scale is read"
    assert torch.equal(got, clean)


# ---- 5. plan recall on a synthetic mass ------------------------------------------------------------------------------------
LN, LLENS = 4480, [4480, 4097, 4096, 300, 0]   # 70 tiles: two steps of the wave; one row into tile 64; exactly 64 tiles; 5; none


def _recall_maps(B, n, lens):
    """all-ones; random at densities 0.5 and 0.03; one that leaves q-blocks of the shortened batches only tiles beyond their
    length (and one with a single tile exactly at its last valid tile)"""
    nqb, ntk = 2, _ntk(n)
    beyond = BU.make_map(B, HQ, M, n, 0.5, 33)
    short = [b for b, x in enumerate(lens) if 0 < x < n]
    for b in short:
        nb = _ntk(lens[b])
        if nb < ntk:
            beyond[b, 0, 1] = False
            beyond[b, 0, 1, nb:] = True          # every tile beyond, none below
            beyond[b, 1, 0] = False
            beyond[b, 1, 0, ntk - 1] = True      # the last tile alone
        beyond[b, 2, 1] = False
        beyond[b, 2, 1, nb - 1] = True           # the last valid tile alone
    return {"ones": torch.ones(B, HQ, nqb, ntk, dtype=torch.bool), "half": BU.make_map(B, HQ, M, n, 0.5, 31),
            "thin": BU.make_map(B, HQ, M, n, 0.03, 32), "beyond": beyond}


@pytest.mark.parametrize("n,lens", [(N, LENS), (LN, LLENS)], ids=["5-tiles", "70-tiles"])
def test_plan_recall_on_a_synthetic_mass(sa, n, lens):
    """the mass is random and NOT zero beyond the lengths: the clip is by list entry"""
    B, ntk = len(lens), _ntk(n)
    mass = torch.rand(B, HQ, 2, ntk, generator=torch.Generator().manual_seed(n)).cuda()
    kv_lens = _lens(lens)
    for name, bm in _recall_maps(B, n, lens).items():
        bmg = bm.cuda()
        plan = sa.block_sparse_plan(bmg, M, n)
        lists = plan.lists.clone()
        for form, arg in (("map", bmg), ("uint8", bmg.to(torch.uint8)), ("plan", plan)):
            rec, kept = sa.plan_recall_kvlen(arg, mass, kv_lens)
            torch.cuda.synchronize()
            assert rec.dtype == torch.float32 and kept.dtype == torch.int32 and tuple(rec.shape) == tuple(kept.shape) == (B, HQ, 2)
            for b, x in enumerate(lens):
                nb = _ntk(x)
                assert torch.equal(kept[b].cpu().long(), bm[b, :, :, :nb].sum(-1)), f"{name} as {form}, batch {b}: kept"
                if x == 0:
                    assert torch.equal(rec[b], torch.zeros_like(rec[b]))
                    continue
                want, wkept = sa.plan_recall(bmg[b:b + 1, :, :, :nb], mass[b:b + 1, :, :, :nb].contiguous())
                assert torch.equal(rec[b:b + 1], want), f"{name} as {form}, batch {b} (len {x}): recall"
                assert torch.equal(kept[b:b + 1], wkept)
        assert torch.equal(plan.lists, lists), "the lists are read-only"
        if name == "beyond":
            b = next(b for b, x in enumerate(lens) if 0 < x and _ntk(x) < ntk)
            assert float(rec[b, 0, 1]) == 0.0 and int(kept[b, 0, 1]) == 0 and float(rec[b, 1, 0]) == 0.0 and int(kept[b, 1, 0]) == 0
            assert float(rec[b, 2, 1]) == float(mass[b, 2, 1, _ntk(lens[b]) - 1]) and int(kept[b, 2, 1]) == 1


# ---- 6. tuning equals brute force ------------------------------------------------------------------------------------------
STEPS = G.STEPS
TN = SU.CASES[G.TUNE_CASE][2]                  # 613 keys: ten tiles, the last of 37 keys
TLENS = [TN, 540, 65, 0]                       # full; inside the last-but-one tile (keys 512 .. 575); one row into tile 1; none


@functools.lru_cache(maxsize=None)
def tune_inputs():
    """the clustered inputs of tests/test_calib_gpu.py batched to B = 4 (the second pair with the heads in reverse order), K
    rows >= len_b NaN; simthreshd1 as there; the length-aware mean and mass.  Do not modify: shared."""
    import sageattention_amd as sa
    from sageattention_amd import _lib as L
    from sageattention_amd.quant import k_smooth_quant_kvlen
    qg, kg, r, _ = G.tune_case()
    q = torch.cat([qg, qg.flip(1)]).contiguous()
    k = _poison(torch.cat([kg, kg.flip(1)]).contiguous(), TLENS)
    kv_lens = _lens(TLENS)
    km = k_smooth_quant_kvlen(k, kv_lens, "HND", L.GRAN_PER_THREAD, L.ROUND_TRITON)[2]
    return q, k, kv_lens, r.simthr, km, sa.sageattn_tile_mass_kvlen(q, k, kv_lens)


@functools.lru_cache(maxsize=None)
def brute_table(rule, reduce):
    """[16, Hq] head recall and density at every grid value, from the public sparge_plan(kv_lens=) + plan_recall_kvlen,
    reduced in fp32 on the device with the expressions sparge_tune_kvlen documents, so that equality is exact"""
    import sageattention_amd as sa
    q, k, kv_lens, simthr, km, mass = tune_inputs()
    Mq = q.shape[2]
    nqb = (Mq + 127) // 128
    weight = C.valid_rows(Mq).float().cuda().view(1, 1, -1)
    lens = kv_lens.clamp(0, TN)
    valid = lens > 0
    nv = valid.sum()
    ntk_b = (lens + 63) // 64
    rows, dens = [], []
    for g in range(1, (1 << STEPS) + 1):
        kw = dict(cdfthreshd=g / 16) if rule == "cdf" else dict(topk=g / 16)
        plan = sa.sparge_plan(q, k, simthreshd1=simthr, keep_first=1, km=km, kv_lens=kv_lens, **kw)
        rec, kept = sa.plan_recall_kvlen(plan, mass, kv_lens)
        if reduce == "mean":
            head = (rec * weight * valid[:, None, None]).sum((0, 2)) * (nv.clamp(min=1) * Mq).to(torch.float32).reciprocal()
        else:
            head = torch.where(valid[:, None, None], rec, INF).amin((0, 2))
        rows.append(head)
        dens.append(kept.sum((0, 2)).to(torch.float32) * (nqb * ntk_b.sum()).clamp(min=1).to(torch.float32).reciprocal())
    return torch.stack(rows), torch.stack(dens)


def _check_tuning(t, rule, reduce, target):
    table, dens = brute_table(rule, reduce)
    param, met, rec, below, _ = C.tune(lambda g: table[g - 1], STEPS, target)
    print(f"tune kvlen {rule} {reduce} target {target}: param = {t.param.tolist()}, met = {t.met.tolist()}, "
          f"recall = {t.recall.tolist()}, below = {t.recall_below.tolist()}, density = {t.density.tolist()}")
    assert t.rule == rule and all(x.is_cuda and tuple(x.shape) == (table.shape[1],) for x in
                                  (t.param, t.met, t.recall, t.recall_below, t.density))
    assert torch.equal(t.param, param) and torch.equal(t.met, met)
    assert torch.equal(t.recall, rec) and torch.equal(t.recall_below, below)
    assert torch.equal(t.density, dens.gather(0, (param * 16).long().view(1, -1) - 1).squeeze(0))
    inner = t.met & (t.param > 2.0 ** -STEPS)
    assert (t.recall_below[inner] < target).all() and (t.recall[inner] >= target).all()
    assert (table[1:] >= table[:-1]).all(), "head recall is monotone in the parameter"


@pytest.mark.parametrize("reduce", ["mean", "min"])
@pytest.mark.parametrize("rule", ["cdf", "topk"])
def test_tune_equals_the_brute_force(sa, rule, reduce):
    q, k, kv_lens, simthr, _, mass = tune_inputs()
    kw = dict(rule=rule, simthreshd1=simthr, keep_first=1, steps=STEPS, reduce=reduce)
    for target in (0.8, 0.95, 1.0):
        _check_tuning(sa.sparge_tune_kvlen(q, k, kv_lens, target=target, **kw), rule, reduce, target)  # computing the mass
        _check_tuning(sa.sparge_tune_kvlen(q, k, kv_lens, target=target, mass=mass, **kw), rule, reduce, target)


def test_plan_recall_kvlen_of_a_plan_made_with_lengths_is_plan_recall(sa):
    """the lists of sparge_plan(kv_lens=) hold no entry >= ntk_b: clipping them changes nothing"""
    q, k, kv_lens, simthr, km, mass = tune_inputs()
    for kw in (dict(cdfthreshd=0.5), dict(topk=0.25, keep_last=1), dict(cdfthreshd=1.0)):
        plan = sa.sparge_plan(q, k, simthreshd1=simthr, km=km, kv_lens=kv_lens, **kw)
        a, b = sa.plan_recall_kvlen(plan, mass, kv_lens), sa.plan_recall(plan, mass)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), kw
        assert int(a[1][3].sum()) == 0 and int(a[1][2].max()) <= 2


# ---- 7. tuning edge cases --------------------------------------------------------------------------------------------------
FIELDS = ("param", "met", "recall", "recall_below", "density")


@pytest.mark.parametrize("reduce", ["mean", "min"])
@pytest.mark.parametrize("rule", ["cdf", "topk"])
def test_tune_with_full_lengths_has_the_bits_of_sparge_tune(sa, rule, reduce):
    qg, kg, r, mass = G.tune_case()
    full = torch.full((qg.shape[0],), TN, dtype=torch.int32, device="cuda")
    kw = dict(target=0.8, rule=rule, simthreshd1=r.simthr, keep_first=1, steps=STEPS, reduce=reduce)
    for m in (None, mass):
        got, want = sa.sparge_tune_kvlen(qg, kg, full, mass=m, **kw), sa.sparge_tune(qg, kg, mass=m, **kw)
        for name in FIELDS:
            assert torch.equal(getattr(got, name), getattr(want, name)), (name, getattr(got, name), getattr(want, name))
        print(f"tune full lengths {rule} {reduce}: param = {want.param.tolist()}, recall = {want.recall.tolist()}")


@pytest.mark.parametrize("reduce", ["mean", "min"])
def test_tune_without_any_key(sa, reduce):
    q, k, _, simthr, _, _ = tune_inputs()
    none = torch.tensor([0, -3, 0, 0], dtype=torch.int32, device="cuda")
    t = sa.sparge_tune_kvlen(q, torch.full_like(k, float("nan")), none, target=0.95, simthreshd1=simthr, steps=STEPS, reduce=reduce)
    Hq = q.shape[1]
    assert torch.equal(t.param, torch.full((Hq,), 2.0 ** -STEPS, device="cuda")) and t.met.all()
    assert torch.equal(t.recall, torch.ones(Hq, device="cuda")) and torch.equal(t.density, torch.zeros(Hq, device="cuda"))
    assert (t.recall_below == -INF).all()


# ---- 8. graph capture ------------------------------------------------------------------------------------------------------
def test_tune_captures_into_a_graph_and_reads_the_lengths_at_replay(sa):
    q, _, _, simthr, _, _ = tune_inputs()
    first, second = TLENS, [100, TN, 0, 300]
    kg = G.tune_case()[1]
    k = _poison(torch.cat([kg, kg.flip(1)]).contiguous(), [max(a, b) for a, b in zip(first, second)])
    kv_lens = _lens(first)
    kw = dict(target=0.8, rule="cdf", simthreshd1=simthr, keep_first=1, steps=STEPS)
    for _ in range(2):
        sa.sparge_tune_kvlen(q, k, kv_lens, **kw)  # warm up: module load
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t_g = sa.sparge_tune_kvlen(q, k, kv_lens, **kw)
    for lens in (second, first):
        kv_lens.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        t_e = sa.sparge_tune_kvlen(q, k, _lens(lens), **kw)
        for name in FIELDS:
            assert torch.equal(getattr(t_g, name), getattr(t_e, name)), (lens, name)
    other = sa.sparge_tune_kvlen(q, k, _lens(second), **kw)
    assert any(not torch.equal(getattr(other, name), getattr(t_e, name)) for name in FIELDS), "the two sets of lengths differ"


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------
def test_tuned_sparse_output_is_within_the_bound_of_the_lost_mass(sa):
    """The bound of tests/test_calib_gpu.py (test_tuned_sparse_output_is_within_the_bound_of_the_lost_mass) on the batches with
    keys: per q-block, mean over its valid rows and over d of |o_sparse - o_dense| <= (2 (1 - recall) + 2^-9) max|v|, with the
    recall of plan_recall_kvlen, the dense operator with the same lengths as the reference, and max|v| over the valid rows."""
    q, k, kv_lens, simthr, _, mass = tune_inputs()
    B, Hq, Mq, D = q.shape
    Hk = k.shape[1]
    v = torch.randn(B, Hk, TN, D, generator=torch.Generator().manual_seed(3)).to(q.dtype).cuda()
    _poison(v, TLENS)
    t = sa.sparge_tune_kvlen(q, k, kv_lens, target=0.95, rule="cdf", simthreshd1=simthr, mass=mass)
    o_s, plan = sa.sageattn_sparge(q, k, v, simthreshd1=simthr, cdfthreshd=t.param, pv="fp16", return_plan=True, kv_lens=kv_lens)
    o_d = sa.sageattn_kvlen(q, k, v, kv_lens, pv="fp16")
    rec, _ = sa.plan_recall_kvlen(plan, mass, kv_lens)
    diff = (o_s.double() - o_d.double()).abs().mean(-1).cpu()  # [B,Hq,M]
    nqb = (Mq + 127) // 128
    per_block = torch.stack([diff[:, :, 128 * i:min(128 * i + 128, Mq)].mean(-1) for i in range(nqb)], -1)
    assert (t.recall[t.met] >= 0.95).all()
    checked = 0
    for b, n in enumerate(TLENS):
        if n == 0:
            assert torch.equal(o_s[b], torch.zeros_like(o_s[b]))
            continue
        vmax = v[b, :, :n].abs().amax((1, 2)).cpu().double().repeat_interleave(Hq // Hk, 0).unsqueeze(-1)  # [Hq,1]
        bound = (2 * (1 - rec[b].cpu().double()).clamp(min=0) + 2.0 ** -9) * vmax
        print(f"end to end kvlen batch {b} (len {n}): max diff / bound = {float((per_block[b] / bound).max()):.4f}, "
              f"min block recall = {float(rec[b].min()):.4f}")
        assert (per_block[b] <= bound).all(), (b, float((per_block[b] / bound).max()))
        checked += 1
    assert checked == 3
    print(f"end to end kvlen: tuned cdfthreshd = {t.param.tolist()}, head recall = {t.recall.tolist()}")
