"""Calibration of the block-map predictor on the GPU: sageattn_tile_mass, plan_recall and sparge_tune against the fp64
restatement of tests/calib_util.py.

Tolerance of the tile mass, |d mass| <= eps * mass + 2^-100, DERIVED from the arithmetic of tile_mass_kernel
(csrc/sage_calib.hip); u = 2^-24, L = max |logit| in base-2 units, ntk = key tiles, every bound first order in u:
  logit      t = float(S) * ((q_scale * logit_mult) * k_scale) with logit_mult = sm_scale * log2 e formed in fp32: S is exact,
             five roundings (the constant, three products of scales, the product with S): |dt| <= 5 u |t| <= 5 u L.
  exponent   the kernel exponentiates t - m with m a computed logit of the same row: |d(t - m)| <= 5 u (|t| + |m|) from the
             logits and u |t - m| from the subtraction, together <= 12 u L; 2^x turns that into a relative 12 ln2 u L.
  v_exp_f32  one ulp: 2 u relative.
             => every exponential of either pass is within a = (12 ln2 L + 2) u of the exact one.
  rescales   pass 1 carries l under a running maximum: l <- l * 2^(m - m') once per tile.  The factor is 1 exactly where the
             maximum stands; elsewhere it has the subtraction's 2 u L ln2, the ulp of v_exp_f32 and the product's rounding:
             <= (2 ln2 L + 3) u per tile, ntk times at most, and once more where the two lane halves of a row are merged.
  sum l      N non-negative terms; in any order the error of such a sum is at most (N - 1) u relative (the kernel's order --
             a tree over a lane's 32, one addition per tile, one for the halves -- is never deeper than 6 ntk + 2).
  p / l      1 / l within 3 u (2.5 ulp), its product with the exponential u.
  tile sum   8192 non-negative terms (128 rows x 64 keys): <= 8191 u by the same crude bound, then the division by c_i, u.
The mass is a ratio of sums of positive terms, so the relative bounds of numerator and denominator add:
  eps = [2 (12 ln2 L + 2) + (ntk + 1) (2 ln2 L + 3) + max(N, 6 ntk + 2) + 4 + 8192] u
-- 5.8e-4 on the concentrated inputs (L = 27), 5.4e-4 on the random ones (L = 8), 4.9e-4 on the smallest shapes.
tests/test_calib.py shows on the CPU that two planted mistakes exceed it."""
import functools
import math

import pytest
import torch

import blocksparse_util as BU
import calib_util as C
import pvskip_util as PU
import sparge_util as SU

pytestmark = pytest.mark.gpu
u = 2.0 ** -24
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)

MAIN = (2, 2, 1, 200, 616)  # B, Hq, Hk, M, N: a ragged q-block (one wave partly, one wholly beyond M), 10 tiles, the last of 40 keys
SMALL = ((1, 40), (129, 64))  # (M, N): one row and one ragged tile; a second q-block of one row and no ragged tile


def eps_for(logits, N):
    """the relative tolerance derived above, for fp64 logits in natural-log units"""
    L = float(logits.abs().max()) * LOG2E
    ntk = (N + 63) // 64
    return (2 * (12 * LN2 * L + 2) + (ntk + 1) * (2 * LN2 * L + 3) + max(N, 6 * ntk + 2) + 4 + 8192) * u


def tolerance(ref, logits, N):
    return eps_for(logits, N) * ref + 2.0 ** -100


@functools.lru_cache(maxsize=None)
def inputs(kind, D, dtype, M, N):
    """q [B,2,M,D], k [B,1,N,D] (HND, CPU): "firm" = the concentrated inputs of the P.V-skip tests, "normal" = random"""
    B = MAIN[0]
    if kind == "firm":
        q, k, _ = PU.make_inputs(B, D, dtype, seed=300 + D, M=M, N=N)
        return q, k
    g = torch.Generator().manual_seed(17 + D + M)
    return torch.randn(B, 2, M, D, generator=g).to(dtype), torch.randn(B, 1, N, D, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def reference(kind, D, gran, dtype, M, N):
    """-> (logits fp64 [B,Hq,M,N], mass fp64 [B,Hq,nqb,ntk]).  Do not modify: shared."""
    q, k = inputs(kind, D, dtype, M, N)
    logits = PU.scaled_logits(q, k, gran)
    return logits, C.tile_mass(logits, M, N)


def _gpu_mass(q, k, gran, layout):
    import sageattention_amd as sa
    qg, kg = q.cuda(), k.cuda()
    if layout == "NHD":
        qg, kg = qg.transpose(1, 2).contiguous(), kg.transpose(1, 2).contiguous()
    return sa.sageattn_tile_mass(qg, kg, tensor_layout=layout, qk_quant_gran=gran)


def _check_mass(kind, D, gran, dtype, layout, M, N):
    q, k = inputs(kind, D, dtype, M, N)
    logits, ref = reference(kind, D, gran, dtype, M, N)
    mass = _gpu_mass(q, k, gran, layout)
    assert mass.dtype == torch.float32 and tuple(mass.shape) == tuple(ref.shape)
    got = mass.cpu().double()
    tol = tolerance(ref, logits, N)
    err = (got - ref).abs()
    print(f"tile mass {kind} D={D} {gran} {dtype} {layout} M={M} N={N}: eps = {eps_for(logits, N):.3e}, "
          f"max err / tol = {float((err / tol).max()):.4f}, max |row sum - 1| = {float((got.sum(-1) - 1).abs().max()):.3e}")
    assert (err <= tol).all(), float((err / tol).max())
    assert ((got.sum(-1) - 1).abs() <= eps_for(logits, N)).all()


@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["firm", "normal"])
def test_tile_mass_matches_the_restatement(kind, D, gran, dtype, layout):
    _check_mass(kind, D, gran, dtype, layout, MAIN[3], MAIN[4])


@pytest.mark.parametrize("MN", SMALL, ids=lambda mn: f"{mn[0]}x{mn[1]}")
@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", ["firm", "normal"])
def test_tile_mass_on_the_smallest_shapes(kind, D, gran, MN):
    _check_mass(kind, D, gran, torch.float16, "HND", *MN)


@pytest.mark.parametrize("gran", ["per_warp", "per_thread"])
@pytest.mark.parametrize("D", [64, 128])
def test_zero_q_spreads_the_mass_by_key_count(D, gran):
    """all logits are 0: every key weighs 1 / N, a tile its key count over N"""
    import sageattention_amd as sa
    B, Hq, Hk, M, N = MAIN
    _, k = inputs("normal", D, torch.float16, M, N)
    mass = sa.sageattn_tile_mass(torch.zeros(B, Hq, M, D, dtype=torch.float16, device="cuda"), k.cuda(), qk_quant_gran=gran)
    keys = (N - 64 * torch.arange((N + 63) // 64)).clamp(max=64).double() / N
    err = (mass.cpu().double() - keys).abs() / keys
    print(f"zero q D={D} {gran}: max relative error = {float(err.max()):.3e} (bound {2.0 ** -20:.3e})")
    assert (err <= 2.0 ** -20).all()


def test_every_entry_is_written_and_two_calls_agree_bit_for_bit():
    from sageattention_amd import _lib as L, core
    B, Hq, Hk, M, N = MAIN
    q, k = (t.cuda() for t in inputs("firm", 64, torch.float16, M, N))
    k8, ks, km = core._prep_k(k, "HND", "per_thread", True)
    q8, qs, _ = core._quant_q(q, km, "HND", "per_thread", 0.125, 32, False, Hq, Hk)
    out = []
    for _ in range(2):
        mass = torch.full((B, Hq, 2, 10), float("nan"), dtype=torch.float32, device="cuda")
        st = L.lib().sage_attn_tile_mass(L.desc(q8, "HND"), L.desc(k8, "HND"), qs.data_ptr(), ks.data_ptr(), B, Hq, Hk, M, N, 64,
                                         L.GRAN_PER_THREAD, 128, 32, 0.125, 0, mass.data_ptr(), L.stream_ptr(q.device))
        assert st == 0
        out.append(mass)
    torch.cuda.synchronize()
    assert not torch.isnan(out[0]).any()
    assert torch.equal(out[0], out[1])
    import sageattention_amd as sa
    assert torch.equal(out[0], sa.sageattn_tile_mass(q, k))  # the public function is this call


# ---- plan recall ------------------------------------------------------------------------------------------------------------
def _recall_case(mass, bm):
    import sageattention_amd as sa
    ntk = mass.shape[-1]
    ref, ref_kept = C.recall(bm, mass.cpu().double())
    for arg in (bm.cuda(), bm.cuda().to(torch.uint8), sa.block_sparse_plan(bm.cuda(), mass.shape[2] * 128, ntk * 64)):
        rec, kept = sa.plan_recall(arg, mass)
        assert rec.dtype == torch.float32 and kept.dtype == torch.int32 and tuple(rec.shape) == tuple(mass.shape[:3])
        assert torch.equal(kept.cpu().long(), ref_kept)
        err = (rec.cpu().double() - ref).abs()
        print(f"plan recall ntk={ntk}: max err / tol = {float((err / (ntk * u * ref + 1e-300)).max()):.4f}")
        assert (err <= ntk * u * ref).all()
    return rec


def test_plan_recall_on_the_gpus_own_mass():
    import sageattention_amd as sa
    B, Hq, Hk, M, N = MAIN
    q, k = (t.cuda() for t in inputs("normal", 64, torch.float16, M, N))
    mass = sa.sageattn_tile_mass(q, k)
    for density, seed in ((0.5, 1), (0.15, 2), (1.0, 3)):
        bm = BU.make_map(B, Hq, M, N, density, seed)
        bm[1, 0, 1] = False  # an empty row: recall 0, kept 0
        rec = _recall_case(mass, bm)
        assert float(rec[1, 0, 1]) == 0.0


@pytest.mark.parametrize("density", [0.5, 0.03])
def test_plan_recall_beyond_one_step_of_the_wave(density):
    """150 tiles: three 64-tile steps, and with the thin map list entries of one step that sit far apart in the list"""
    mass = torch.rand(2, 3, 2, 150, generator=torch.Generator().manual_seed(5)).cuda()
    bm = BU.make_map(2, 3, 256, 150 * 64, density, 11)
    bm[0, 2, 0] = False
    _recall_case(mass, bm)


def test_plan_recall_refuses_what_does_not_fit():
    import sageattention_amd as sa
    mass = torch.rand(2, 2, 2, 10).cuda()
    with pytest.raises(ValueError):
        sa.plan_recall(torch.ones(2, 2, 2, 9, dtype=torch.bool, device="cuda"), mass)
    with pytest.raises(ValueError):
        sa.plan_recall(sa.block_sparse_plan(torch.ones(2, 2, 3, 10, dtype=torch.bool, device="cuda"), 300, 616), mass)
    with pytest.raises(ValueError):
        sa.plan_recall(torch.ones(2, 2, 2, 10, dtype=torch.bool, device="cuda"), mass.double())


# ---- tune -------------------------------------------------------------------------------------------------------------------
TUNE_CASE, STEPS = "c1", 4


@functools.lru_cache(maxsize=None)
def tune_case():
    """the clustered inputs on the GPU, simthreshd1 from the fp64 statistics (as tests/test_sparge_gpu.py), the exact mass"""
    import sageattention_amd as sa
    from sageattention_amd import quant
    q, k = SU.inputs(TUNE_CASE)
    qg, kg = q.cuda(), k.cuda()
    r = SU.Ref(TUNE_CASE, quant.k_mean(kg).cpu())
    assert r.gap[1] - r.gap[0] >= 0.1, r.gap
    return qg, kg, r, sa.sageattn_tile_mass(qg, kg)


@functools.lru_cache(maxsize=None)
def brute_table(rule, reduce):
    """[16, Hq] head recall and density at every grid value, from the public sparge_plan + plan_recall; reduced in fp32 on
    the device with the expression sparge_tune documents, so that equality is exact"""
    import sageattention_amd as sa
    qg, kg, r, mass = tune_case()
    B, M = qg.shape[0], qg.shape[2]
    w = C.valid_rows(M).float().cuda().view(1, 1, -1)
    rows, dens = [], []
    for g in range(1, (1 << STEPS) + 1):
        kw = dict(cdfthreshd=g / 16) if rule == "cdf" else dict(topk=g / 16)
        rec, kept = sa.plan_recall(sa.sparge_plan(qg, kg, simthreshd1=r.simthr, keep_first=1, **kw), mass)
        rows.append((rec * w).sum(dim=(0, 2)) / float(B * M) if reduce == "mean" else rec.amin(dim=(0, 2)))
        dens.append(kept.sum(dim=(0, 2)).float() / float(kept.shape[0] * kept.shape[2] * mass.shape[3]))
    return torch.stack(rows), torch.stack(dens)


def _check_tuning(t, rule, reduce, target):
    table, dens = brute_table(rule, reduce)
    param, met, rec, below, _ = C.tune(lambda g: table[g - 1], STEPS, target)
    print(f"tune {rule} {reduce} target {target}: param = {t.param.tolist()}, met = {t.met.tolist()}, recall = {t.recall.tolist()}, "
          f"below = {t.recall_below.tolist()}, density = {t.density.tolist()}")
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
def test_tune_equals_the_brute_force(rule, reduce):
    import sageattention_amd as sa
    qg, kg, r, mass = tune_case()
    for target in (0.8, 0.95, 1.0):  # (on these inputs the CDF rule needs 1.0 for 0.95; 0.8 ends inside the grid)
        t = sa.sparge_tune(qg, kg, target=target, rule=rule, simthreshd1=r.simthr, keep_first=1, steps=STEPS, reduce=reduce,
                           mass=mass)
        _check_tuning(t, rule, reduce, target)
    t = sa.sparge_tune(qg, kg, target=0.95, rule=rule, simthreshd1=r.simthr, keep_first=1, steps=STEPS, reduce=reduce)
    _check_tuning(t, rule, reduce, 0.95)  # ... computing the mass itself


def test_tune_captures_into_a_graph():
    import sageattention_amd as sa
    qg, kg, r, _ = tune_case()
    q, k = qg.clone(), kg.clone()
    kw = dict(target=0.95, rule="cdf", simthreshd1=r.simthr, keep_first=1, steps=STEPS)
    for _ in range(2):
        sa.sparge_tune(q, k, **kw)  # warm up: module load
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t_g = sa.sparge_tune(q, k, **kw)
    for step in (0, 1):  # the captured values, then the batches swapped
        if step:
            q.copy_(qg.flip(0)); k.copy_(kg.flip(0))
        g.replay()
        torch.cuda.synchronize()
        t_e = sa.sparge_tune(q, k, **kw)
        for name in ("param", "met", "recall", "recall_below", "density"):
            assert torch.equal(getattr(t_g, name), getattr(t_e, name)), name


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_tuned_sparse_output_is_within_the_bound_of_the_lost_mass():
    """Per q-block, mean over its valid rows and over d of |o_sparse - o_dense| <= 2 (1 - recall) max|v| + 2^-9 max|v|: a row
    that keeps the share R of its probability renormalises the kept part by 1 / R (moving it by at most 1 - R in units of
    max|v|) and drops the rest (1 - R again), and recall is the mean of R over the block's rows; 2^-9 max|v| covers the fp16
    roundings of P and o in both operators."""
    import sageattention_amd as sa
    qg, kg, r, mass = tune_case()
    D, M, N, Hq, Hk, B, dtype = SU.CASES[TUNE_CASE]
    v = torch.randn(B, Hk, N, D, generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
    t = sa.sparge_tune(qg, kg, target=0.95, rule="cdf", simthreshd1=r.simthr, mass=mass)
    o_s, plan = sa.sageattn_sparge(qg, kg, v, simthreshd1=r.simthr, cdfthreshd=t.param, pv="fp16", return_plan=True)
    o_d = sa.sageattn_qk_int8_pv_fp16_cuda(qg, kg, v, qk_quant_gran="per_thread")
    rec, _ = sa.plan_recall(plan, mass)
    diff = (o_s.double() - o_d.double()).abs().mean(-1).cpu()  # [B,Hq,M]
    nqb = (M + 127) // 128
    per_block = torch.stack([diff[:, :, 128 * i:min(128 * i + 128, M)].mean(-1) for i in range(nqb)], -1)
    vmax = v.abs().amax((2, 3)).cpu().double().repeat_interleave(Hq // Hk, 1).unsqueeze(-1)  # [B,Hq,1]
    bound = (2 * (1 - rec.cpu().double()).clamp(min=0) + 2.0 ** -9) * vmax
    print(f"end to end: tuned cdfthreshd = {t.param.tolist()}, head recall = {t.recall.tolist()}, "
          f"max diff / bound = {float((per_block / bound).max()):.4f}, min block recall = {float(rec.min()):.4f}")
    assert (t.recall[t.met] >= 0.95).all()
    assert (per_block <= bound).all(), float((per_block / bound).max())
