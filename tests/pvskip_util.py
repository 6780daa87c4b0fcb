"""The P.V skip of block-sparse attention (include/sageattn_hip.h, sage_attn_*_blocksparse_pvskip) restated in torch, fp64,
and the inputs its tests use.

The rule: a wave is 32 query rows of a 128-row q-block.  For the tile at list position pos of the q-block's list it skips
iff pos > 0 and, on every row r < M of the wave, t[r] <= m_ref[r] - pvthreshd[h]; t is the row maximum of the tile's scaled
logits over keys < N (natural-log units) and m_ref the kernel's reference maximum, which lags the true running maximum of
the row by at most lazy = kLazyThr ln 2.  The restatement walks the lists with the TRUE running maximum, so it is the kernel's
decision exactly where no wave-tile has a gap inside (pvthreshd - 0, pvthreshd + lazy): the firm inputs below keep every
gap at least 1 away from that band (asserted in tests/test_pvskip.py)."""
import functools
import math

import torch

LN2 = math.log(2.0)
LAZY = {"fp16": 6 * LN2, "fp8": 3 * LN2}  # kLazyThr ln 2 of the FP16 / BF16 and of the FP8 P.V loop

# the firm inputs: M, N (10 key tiles, the last holds 40 keys), one KV head, two query heads
M_FIRM, N_FIRM, HK_FIRM, HQ_FIRM = 200, 616, 1, 2
LX = [0, -60, -60, 0, -60, 0, -60, -60, 0, -60]
LY = [-60, 0, -60, -60, 0, 0, -60, 0, -60, 0]


def make_inputs(B, D, dtype, seed, lx=LX, ly=LY, noise=0.05, M=M_FIRM, N=N_FIRM, sm_scale=None):
    """q [B,2,M,D], k and v [B,1,N,D] (HND, CPU).  q rows are A e_axis + noise randn with A = 0.5 / sm_scale, so a key at
    level L along the row's axis has the scaled logit 0.5 L whatever the head_dim.  Head 0: axis (row // 32) % 2, except
    rows 96..127 whose axis alternates by row (a wave whose halves disagree); head 1: axis 1.  Keys of tile j are
    lx[j] e_0 + ly[j] e_1 + noise randn; v is randn."""
    g = torch.Generator().manual_seed(seed)
    sm_scale = D ** -0.5 if sm_scale is None else sm_scale
    A = 0.5 / sm_scale
    rows = torch.arange(M)
    axis0 = (rows // 32) % 2
    axis0 = torch.where((rows >= 96) & (rows < 128), rows % 2, axis0)
    axis = torch.stack([axis0, torch.ones(M, dtype=torch.long)])                # [2, M]
    q = noise * torch.randn(B, HQ_FIRM, M, D, generator=g)
    q += A * torch.nn.functional.one_hot(axis, D).to(q.dtype).unsqueeze(0)
    tile = torch.arange(N) // 64
    k = noise * torch.randn(B, HK_FIRM, N, D, generator=g)
    k[..., 0] += torch.tensor(lx, dtype=k.dtype)[tile]
    k[..., 1] += torch.tensor(ly, dtype=k.dtype)[tile]
    v = torch.randn(B, HK_FIRM, N, D, generator=g)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def list_map(B, Hq, M, N, lengths):
    """bool map [B,Hq,ceil(M/128),ceil(N/64)] whose list rows, in (b, h, q-block) order, have the given lengths: an even
    length takes the first tiles, an odd one the first length - 1 and the last (ragged) tile."""
    nqb, ntk = (M + 127) // 128, (N + 63) // 64
    assert len(lengths) == B * Hq * nqb
    bm = torch.zeros(B * Hq * nqb, ntk, dtype=torch.bool)
    for i, n in enumerate(lengths):
        if n % 2 == 0:
            bm[i, :n] = True
        else:
            bm[i, :n - 1] = True
            bm[i, ntk - 1] = True
    return bm.view(B, Hq, nqb, ntk)


# list lengths of the eight list rows of the firm configuration (B = 2): both ring depths, every remainder of the unrolled
# fast loops, and both tail forms (a ragged last tile for the odd lengths, a plain one for the even ones)
FIRM_LENGTHS = [10, 9, 7, 6, 5, 3, 2, 1]


def scaled_logits(q, k, gran, sm_scale=None):
    """fp64 [B,Hq,M,N]: the logits the kernel exponentiates, in natural-log units -- the oracle's INT8 Q and smoothed K and
    their scales, composed as _oracle of tests/test_block_sparse_gpu.py composes them (HND, CPU)."""
    from oracle import sage_oracle as O
    D = q.shape[-1]
    sm_scale = D ** -0.5 if sm_scale is None else sm_scale
    km = O.k_mean(k, "HND")
    quant = O.per_thread_int8 if gran == "per_thread" else O.per_warp_int8
    q8, qs, k8, ks = quant(q, k, km, tensor_layout="HND")
    M, N = q8.shape[2], k8.shape[2]
    qrows, kcols = O.expand_q_scale(qs, M, gran).double(), O.expand_k_scale(ks, N, gran).double()
    grp = q8.shape[1] // k8.shape[1]
    k8 = k8.repeat_interleave(grp, dim=1).double()
    kcols = kcols.repeat_interleave(grp, dim=1)
    s = q8.double() @ k8.transpose(-1, -2)
    return s * qrows.unsqueeze(-1) * kcols.unsqueeze(-2) * sm_scale


def restate(logits, bm, pvthreshd):
    """The rule on fp64 logits [B,Hq,M,N] (natural-log units), the bool map bm and per-head thresholds (a float or a
    sequence of Hq floats; values that are not > 0, inf and NaN never skip).
    -> (skipped, counts, min_skip_gap, max_keep_gap):
      skipped[(b, h, i, w)]  the set of skipped list POSITIONS of wave w of q-block i
      counts                 int32 [B,Hq,ceil(M/128),4], their sizes (0 for a wave without a row < M)
      min_skip_gap           the smallest gap of a skipped wave-tile, max_keep_gap the largest of one at pos > 0 that is kept
                             (heads with a finite threshold);
                             the gap of a wave-tile is min over the wave's rows < M of (true running maximum - t)"""
    B, Hq, M, N = logits.shape
    nqb, ntk = (M + 127) // 128, (N + 63) // 64
    thr = [float(pvthreshd)] * Hq if not hasattr(pvthreshd, "__len__") else [float(x) for x in pvthreshd]
    thr = [t if (t > 0 and math.isfinite(t)) else math.inf for t in thr]
    bm = bm.expand(B, Hq, nqb, ntk)
    skipped, counts = {}, torch.zeros(B, Hq, nqb, 4, dtype=torch.int32)
    min_skip, max_keep = math.inf, -math.inf
    for b in range(B):
        for h in range(Hq):
            for i in range(nqb):
                tiles = torch.nonzero(bm[b, h, i]).flatten().tolist()
                for w in range(4):
                    r0, r1 = 128 * i + 32 * w, min(128 * i + 32 * w + 32, M)
                    skipped[(b, h, i, w)] = set()
                    if r0 >= M:
                        continue
                    m = torch.full((r1 - r0,), -math.inf, dtype=torch.float64)
                    for pos, j in enumerate(tiles):
                        t = logits[b, h, r0:r1, 64 * j:min(64 * j + 64, N)].amax(-1)
                        if pos > 0:
                            gap = (m - t).min().item()
                            if gap >= thr[h]:
                                skipped[(b, h, i, w)].add(pos)
                                min_skip = min(min_skip, gap)
                                continue  # a skipped tile changes nothing
                            if math.isfinite(thr[h]):  # (a head that never skips keeps every gap, firmly)
                                max_keep = max(max_keep, gap)
                        m = torch.maximum(m, t)
                    counts[b, h, i, w] = len(skipped[(b, h, i, w)])
    return skipped, counts, min_skip, max_keep


def map_without(bm, skipped, w):
    """bm (bool [B,Hq,nqb,ntk]) with the tiles that wave w of each q-block skipped switched off"""
    out = bm.clone()
    for (b, h, i, ww), positions in skipped.items():
        if ww != w:
            continue
        tiles = torch.nonzero(bm[b, h, i]).flatten().tolist()
        for pos in positions:
            out[b, h, i, tiles[pos]] = False
    return out


def wave_rows(M, w):
    """bool [M]: the rows that belong to wave w of their q-block"""
    return (torch.arange(M) % 128) // 32 == w


@functools.lru_cache(maxsize=None)
def firm_case(D, gran, dtype, thr=16.0, B=2):
    """The firm configuration of the GPU tests for one (head_dim, granularity, dtype): inputs, map, restatement."""
    q, k, v = make_inputs(B, D, dtype, seed=1000 + D)
    bm = list_map(B, HQ_FIRM, M_FIRM, N_FIRM, FIRM_LENGTHS)
    logits = scaled_logits(q, k, gran)
    return (q, k, v, bm, logits) + restate(logits, bm, thr)


# Inputs that are NOT firm, for the error bound: tiles whose scaled logits lie at the levels {0, -12, -24, -36} below the best
# one (key levels twice that: a key at level L has the scaled logit 0.5 L), noise 0.5, against pvthreshd = 20.  Gaps of 12
# never skip, gaps of 36 do, and gaps of 24 +- noise fall on either side of the threshold and inside the lazy band.
LOOSE_LOGIT_LEVELS = [0, -12, -24, -36]


@functools.lru_cache(maxsize=None)
def loose_case(D, gran, dtype, B=1, seed=7):
    g = torch.Generator().manual_seed(seed)
    lv = 2 * torch.tensor(LOOSE_LOGIT_LEVELS)
    lx = lv[torch.randint(0, 4, (10,), generator=g)].tolist()
    ly = lv[torch.randint(0, 4, (10,), generator=g)].tolist()
    q, k, v = make_inputs(B, D, dtype, seed=seed + D, lx=lx, ly=ly, noise=0.5)
    bm = torch.ones(B, HQ_FIRM, 2, 10, dtype=torch.bool)
    return q, k, v, bm, scaled_logits(q, k, gran)
