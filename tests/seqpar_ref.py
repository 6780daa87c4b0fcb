"""Plain fp64 references of the sequence-parallel building blocks (sage_seq_stats, sage_kv_stats_reduce, the state merges,
sage_finish_lse), the case table of the merge tests and the error bounds the GPU tests assert.  numpy / torch on the CPU
only: no GPU, no oracle.  Test infrastructure (tests/test_seqpar_ref.py checks it against the CPU stand-ins of
tests/ring_cpu_backend.py; tests/test_seqpar_blocks_gpu.py and tests/test_seqpar_backends_gpu.py check the kernels against it)."""
from collections import namedtuple

import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
LOG2E32 = np.float32(1.44269504)

# Relative error of the device's fast exp / log pair (__expf, __logf) on arguments in [-104, 0], as it shows in a merge:
# the one constant of the merge bounds that cannot be derived from the number formats.  Measured once on kind (a) rows
# against merge_ref (profiles/seqpar_blocks.md: 3.6e-7 = 2^-21.4 needed at most), rounded up to a power of two (2^-21)
# and given a factor 4 for the spread between inputs.  The tests read it from here, never from a run of the kernel.
EPS_EXP = 2.0 ** -19


# ----------------------------------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------------------------------

def stats_ref(x):
    """fp64 (max, min, sum, sum_abs) per channel of x [B,H,N,D] (any strides) over its N rows: four [B,H,D] tensors."""
    xd = x.detach().cpu().double()
    return xd.amax(2), xd.amin(2), xd.sum(2), xd.abs().sum(2)


def sum_additions(n_rows, D, parts=0):
    """Number of fp32 additions on the longest path from an element to its channel sum, counted from the kernels
    (sageattention_amd/csrc/sage_fp8.hip; VQ_ROWS: sage_fp8_kernels.h):
      rows per thread        VQ_ROWS / RPP = D / 8     v_stats_partial_kernel, `sm[j] += f[j]` (lines 36 / 47; VQ_ROWS = 256,
                                                       TPR = D / 8 threads per row, RPP = 256 / TPR rows per pass)
      workgroup pass         RPP - 1 = 2048 / D - 1    same kernel, `e += red[2][r][..]` for r = 1 .. RPP-1 (line 58)
      chunks                 S = ceil(N / 256)         seq_stats_final_kernel, `e += ve[u]` (line 132)
      shards                 parts                     kv_stats_reduce_kernel, `sum += ks[..]` (line 149)
    The first addition of the thread loop, of the chunk loop and of the shard loop adds to 0.0f and is exact; counting them
    anyway covers the second-order terms of (1 + u)^A - 1, so |err| <= A * 2^-24 * sum|x| holds as stated."""
    return D // 8 + (2048 // D - 1) + -(-n_rows // 256) + parts


def sum_bound(sum_abs, n_rows, D, parts=0):
    """|fp32 sum - exact sum| <= A * 2^-24 * sum|x| (every partial sum is at most sum|x| in magnitude; inputs are fp16/bf16,
    exact in fp32)."""
    return sum_additions(n_rows, D, parts) * U32 * sum_abs


def ulp(x, dtype):
    """Spacing of ``dtype`` (fp16 / bf16 / fp32) at |x| (fp64 tensor), subnormal spacing below the smallest normal."""
    mant, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dtype]
    ax = x.abs().double()
    e = torch.floor(torch.log2(torch.where(ax > 0, ax, torch.ones_like(ax)))).clamp(min=emin)
    e = torch.where(ax > 0, e, torch.full_like(e, emin))
    return torch.pow(torch.full_like(e, 2.0), e - mant)


ReduceRef = namedtuple("ReduceRef", "mean amax v_scale v_coef")


def reduce_ref(all_stats, n_total, dtype, scale_max=448.0):
    """all_stats fp32 [P][c][BH][3][D] (c = 1: K only; 2: K, V) -> fp64 mean [BH,D] of K over n_total rows and, with V,
    amax, v_scale = amax / scale_max and v_coef = scale_max / amax as SINGLE IEEE fp32 divisions (numpy float32 arrays),
    0 where amax == 0 (a channel that is zero over the whole sequence).  ``dtype`` is the storage type of km (the caller
    rounds: the mean is returned unrounded for the half-ulp bound)."""
    st = all_stats.detach().cpu()
    mean = st[:, 0, :, 2, :].double().sum(0) / float(n_total)
    if st.shape[1] < 2:
        return ReduceRef(mean, None, None, None)
    vmax = st[:, 1, :, 0, :].amax(0).numpy().astype(np.float32)
    vmin = st[:, 1, :, 1, :].amin(0).numpy().astype(np.float32)
    amax = np.maximum(np.abs(vmax), np.abs(vmin))
    sm = np.full_like(amax, np.float32(scale_max))
    v_scale = amax / sm
    with np.errstate(divide="ignore"):
        v_coef = np.where(amax > 0, sm / amax, np.float32(0)).astype(np.float32)
    return ReduceRef(mean, torch.from_numpy(amax), torch.from_numpy(v_scale), torch.from_numpy(v_coef))


# ----------------------------------------------------------------------------------------------------------------------
# merges
# ----------------------------------------------------------------------------------------------------------------------

MergeRef = namedtuple("MergeRef", "o lse wabs lmax")


def merge_ref(os_, lses, in_mult=1.0, corr=None, corr_mult=0.0):
    """fp64 logsumexp merge of the block results (o_i [rows,D], l_i [rows]):
        l_i' = l_i * in_mult;  lse = log sum_i exp(l_i') (+ corr * corr_mult);  o = sum_i o_i exp(l_i' - logsumexp).
    A block with l_i = -inf is empty: it weighs 0 WHATEVER its o holds (NaN, Inf).  All blocks empty: (0, -inf).
    in_mult / corr_mult are taken at their fp32 values (what the kernel is handed).  Also returned for the bounds:
    wabs = sum_i w_i |o_i| and lmax = max_i |l_i'| over the non-empty blocks (0 where there is none)."""
    im, cm = float(np.float32(in_mult)), float(np.float32(corr_mult))
    l = torch.stack([t.detach().cpu().double() for t in lses]) * im                    # [P,rows]
    o = torch.stack([t.detach().cpu().double() for t in os_])                          # [P,rows,D]
    empty = torch.isinf(l) & (l < 0)
    mx = l.amax(0)
    some = ~torch.isinf(mx)
    e = torch.where(empty | ~some, torch.zeros_like(l), torch.exp(l - torch.where(some, mx, torch.zeros_like(mx))))
    s = e.sum(0)
    w = e / torch.where(some, s, torch.ones_like(s))
    oz = torch.where(empty.unsqueeze(-1), torch.zeros_like(o), o)
    out = (oz * w.unsqueeze(-1)).sum(0)
    wabs = (oz.abs() * w.unsqueeze(-1)).sum(0)
    lse = torch.where(some, mx + torch.log(torch.where(some, s, torch.ones_like(s))), torch.full_like(mx, float("-inf")))
    if corr is not None:
        lse = lse + corr.detach().cpu().double() * cm
    lmax = torch.where(empty, torch.zeros_like(l), l.abs()).amax(0)
    return MergeRef(out, lse, wabs, lmax)


def merge_eps(ref):
    """eps of the merge bounds, per row: EPS_EXP + 3 * 2^-24 * (1 + max_i |l_i * in_mult|).  The second term is the fp32
    rounding of the scaled LSE (l_i * in_mult), of the shifted exponent argument (l_i' - max) and of max + log(sum); it
    dominates when the LSEs carry a large common offset."""
    return EPS_EXP + 3 * U32 * (1 + ref.lmax)


def merge_tolerances(ref, out_dtype, roundings=1):
    """(o_tol [rows,D], lse_tol [rows]):  |o - ref| <= roundings * ulp_out(ref)/2 + eps * sum_i w_i|o_i|,
    |lse - ref| <= eps + 2^-23 |ref|.  out_dtype None: an fp32 accumulator, no output ulp (roundings = 0)."""
    eps = merge_eps(ref)
    o_tol = eps.unsqueeze(-1) * ref.wabs
    if out_dtype is not None:
        o_tol = o_tol + roundings * 0.5 * ulp(ref.o, out_dtype)
    fin = ~torch.isinf(ref.lse)
    lse_tol = eps + 2.0 ** -23 * torch.where(fin, ref.lse.abs(), torch.zeros_like(ref.lse))
    return o_tol, lse_tol


def finish_lse_ref(lse2, corr, sm_scale):
    """sage_finish_lse in numpy float32: `lse2 / 1.44269504f`, then `+ corr * sm_scale` with the product and the sum rounded
    separately (core.py:651 as torch evaluates it).  lse2 / corr: fp32 tensors; returns an fp32 tensor."""
    v = lse2.detach().cpu().numpy().astype(np.float32) / LOG2E32
    if corr is not None:
        p = corr.detach().cpu().numpy().astype(np.float32) * np.float32(sm_scale)
        v = (v + p).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))


# ----------------------------------------------------------------------------------------------------------------------
# the case table of the merge tests
# ----------------------------------------------------------------------------------------------------------------------

# (a) LSEs ~ 3 N(0,1)                                      (b) all LSEs equal and all o_i equal
# (c) one block >= 110 nats above the rest, placed first / in the middle / last: fp32 exp(-110) is 0, so that block comes
#     back bit for bit and lse equals its LSE
# (d) kind (a) plus a common offset of +-3e4: the maximum must be subtracted BEFORE the exponential
# (e) -inf in slot 0 / a middle slot / the last slot, those blocks' o filled with NaN and +-Inf
# (f) every slot -inf
KINDS = ("a", "b", "c_first", "c_mid", "c_last", "d_plus", "d_minus", "e_first", "e_mid", "e_last", "f")
DOMINANT_GAP = 110.0

MergeCases = namedtuple("MergeCases", "os lses kind slot")


def kind_slot(name, count):
    """The slot a kind singles out (the dominant block of (c), the empty block of (e)), or -1."""
    if name.endswith("_first"):
        return 0
    if name.endswith("_mid"):
        return count // 2
    if name.endswith("_last"):
        return count - 1
    return -1


def merge_cases(count, rows, D=64, dtype=torch.float16, in_mult=1.0, seed=0):
    """``count`` block results of ``rows`` rows from the fixed menu KINDS: row r is of kind (r + count) % len(KINDS), so
    every table of at least len(KINDS) rows holds every kind.  The menu describes the SCALED LSEs l_i * in_mult (natural
    log); the returned l_i are divided by in_mult.  -> MergeCases(os [count x (rows,D) dtype], lses [count x (rows,) fp32],
    kind [rows] index into KINDS, slot [rows] the singled-out slot or -1).  CPU tensors, deterministic."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * count + 31 * rows + D + (7 if dtype == torch.bfloat16 else 0))
    o = torch.randn(count, rows, D, generator=g).to(dtype)
    l = torch.randn(count, rows, generator=g) * 3
    kind = (torch.arange(rows) + count) % len(KINDS)
    slot = torch.full((rows,), -1, dtype=torch.long)
    poison = torch.tensor([float("nan"), float("inf"), float("-inf")]).to(dtype)
    for ki, name in enumerate(KINDS):
        m = kind == ki
        if not m.any():
            continue
        s = kind_slot(name, count)
        slot[m] = s
        if name == "b":
            l[:, m] = l[0, m]
            o[:, m] = o[0, m]
        elif name.startswith("c_"):
            rest = l[:, m].clone()
            rest[s] = float("-inf")
            top = rest.amax(0) if count > 1 else l[s, m]
            l[s, m] = top + (DOMINANT_GAP + 5.0) + 5.0 * torch.rand(int(m.sum()), generator=g)
        elif name.startswith("d_"):
            l[:, m] += 3e4 if name == "d_plus" else -3e4
        elif name.startswith("e_"):
            l[s, m] = float("-inf")
            n = int(m.sum())
            o[s, m] = poison[(torch.arange(n).view(-1, 1) + torch.arange(D).view(1, -1)) % 3]
        elif name == "f":
            l[:, m] = float("-inf")
            o[0, m] = poison[0]
    if float(np.float32(in_mult)) != 1.0:
        l = (l.double() / float(np.float32(in_mult))).float()
    return MergeCases([o[i].contiguous() for i in range(count)], [l[i].contiguous() for i in range(count)], kind, slot)


# ----------------------------------------------------------------------------------------------------------------------
# the assertions the GPU tests share (CPU tensors in, nothing of the GPU here)
# ----------------------------------------------------------------------------------------------------------------------

def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_stats(st, x):
    """st: fp32 [BH,3,D] from the kernel (CPU), x: the tensor (CPU).  max / min bit-exact (with the zero rows of the 16-row
    padding), the sum within the derived bound."""
    B, H, N, D = x.shape
    mx, mn, sm, sa = (t.view(B * H, D) for t in stats_ref(x))
    if N % 16:                                           # rows [N, ceil16(N)) count as zeros
        true_abs = torch.maximum(mx.abs(), mn.abs())
        mx, mn = mx.clamp(min=0.0), mn.clamp(max=0.0)
        assert torch.equal(torch.maximum(st[:, 0].abs(), st[:, 1].abs()).double(), true_abs)     # max|x| is exact
    assert torch.equal(st[:, 0].double(), mx) and torch.equal(st[:, 1].double(), mn)
    err = (st[:, 2].double() - sm).abs()
    bound = sum_bound(sa, N, D)
    assert (err <= bound).all(), (err / bound).max().item()


def km_tolerance(mean, got, sum_abs, n_shard, D, parts, n_total, dt):
    """|km - fp64 mean| <= half an ulp of the storage type (at the larger of the two magnitudes: a mean just below a power
    of two may round up into the next binade) + the sum bound / n_total + the fp32 division's rounding."""
    big = torch.maximum(mean.abs(), got.abs())
    return 0.5 * ulp(big, dt) + sum_bound(sum_abs, n_shard, D, parts) / n_total + U32 * mean.abs()


def check_merge(o, lse, ref, dt, o_extra=None, passes=1):
    """The toleranced assertions against fp64 (merge_tolerances), NaN-free, -inf exactly where the reference has it.
    passes: merge passes the result went through (the fp32 error terms once per pass; the output ulp once); o_extra: a
    further term of the o bound."""
    o_tol, l_tol = merge_tolerances(ref, None)
    o_tol, l_tol = o_tol * passes + 0.5 * ulp(ref.o, dt), l_tol * passes
    if o_extra is not None:
        o_tol = o_tol + o_extra
    assert not torch.isnan(o.float()).any() and torch.isfinite(o.float()).all()
    if lse is not None:
        assert not torch.isnan(lse).any()
        assert torch.equal(torch.isneginf(lse), torch.isneginf(ref.lse))
        fin = torch.isfinite(ref.lse)
        e = (lse.double() - ref.lse).abs()
        assert (e[fin] <= l_tol[fin]).all(), (e[fin] / l_tol[fin]).max().item()
    e = (o.double() - ref.o).abs()
    assert (e <= o_tol).all(), (e / o_tol.clamp(min=1e-300)).max().item()
