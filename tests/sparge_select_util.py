"""The selection rules of sage_block_select (include/sageattn_hip.h) restated in torch: kept key blocks, candidates, the
TOPK count in float32 exactly as the header states it, a stable descending sort, and the CDF rule over the candidates.
Shared by tests/test_sparge_select.py (CPU) and tests/test_sparge_select_gpu.py; inputs and the fp64 block statistics
come from tests/sparge_util.py.

The reference works in fp64 on fp32 block statistics (on the GPU: the pooling kernel's own outputs), so only the rounding
of the kernel's fp32 dot separates the two.  That dot is D/8 sequential fmas, 3 lane additions and the scale -- never
deeper than D + 1 roundings -- so a score is within
    bound_j = (D + 1) * 2^-24 * sm_scale * sum_d |pq_d| |pk_jd|
of the reference's.  A row is FIRM if its k-th and (k+1)-th candidate scores (k = kcount) differ by more than the sum of
their two bounds; on firm rows the kernel must select exactly the reference's set."""
import torch

import sparge_util as U

TOPKS = (0.125, 0.3, 0.5)
KEEPS = ((0, 0), (2, 1))
NONFIRM_CAP = 1.0 / 16  # share of the live rows of one combination that may be not firm: a condition on the inputs


def kcount(topk, n):
    """topk: float or tensor (any shape), n: int tensor broadcastable to it -> int64 tensor.
    n if !(topk < 1) (1 and above, NaN), else min(n, max(1, (int)ceilf(topk * (float)n))): ONE float32 multiplication."""
    t = torch.as_tensor(topk, dtype=torch.float32)
    n = torch.as_tensor(n, dtype=torch.int64)
    frac = t < 1
    prod = torch.where(frac, t, torch.zeros_like(t)) * n.to(torch.float32)  # float32 * float32 -> float32
    k = torch.minimum(n, torch.clamp(torch.ceil(prod), min=1.0).to(torch.int64))
    return torch.where(frac, k, n.expand_as(k))


def kept(ntk, keep_first, keep_last):
    """bool [ntk]: j < keep_first or j >= ntk - keep_last; values beyond ntk act as ntk."""
    j = torch.arange(ntk)
    return (j < min(keep_first, ntk)) | (j >= ntk - min(keep_last, ntk))


def full_map(sel, cand, selfsim):
    """Tile (i, j) is on if j is selected, or j is not a candidate, or i is not self-similar."""
    return sel | ~cand | ~selfsim


class Rule:
    """The rule on given block statistics (pq [B,Hq,nqb,D], sq [B,Hq,nqb], pk [B,Hk,ntk,D], sk [B,Hk,ntk]; CPU, any float
    dtype), evaluated in fp64.  simthr: float or [Hq]."""

    def __init__(self, pq, sq, pk, sk, sm_scale, simthr):
        g = pq.shape[1] // pk.shape[1]
        self.D = pq.shape[-1]
        self.Hq, self.nqb, self.ntk = pq.shape[1], pq.shape[2], pk.shape[2]
        pq, pk = pq.double(), pk.double().repeat_interleave(g, 1)
        thr = torch.as_tensor(simthr, dtype=torch.float64).reshape(1, -1, 1)
        self.s = (pq @ pk.transpose(-1, -2)) * sm_scale + 0.0          # [B,Hq,nqb,ntk]; -0 -> +0
        self.bound = (self.D + 1) * 2.0 ** -24 * sm_scale * (pq.abs() @ pk.abs().transpose(-1, -2))
        self.elig = (sk.double().repeat_interleave(g, 1) > thr).unsqueeze(2)   # [B,Hq,1,ntk]
        self.selfsim = (sq.double() > thr).unsqueeze(-1)                       # [B,Hq,nqb,1]

    def cand(self, keep_first=0, keep_last=0):
        return self.elig & ~kept(self.ntk, keep_first, keep_last).view(1, 1, 1, -1)

    def live(self, cand):
        """[B,Hq,nqb]: rows in which a selection takes place."""
        return self.selfsim.squeeze(-1) & cand.any(-1)

    def kc(self, cand, topk):
        """[B,Hq,1]: kcount of every (b, h_q)."""
        t = torch.as_tensor(topk, dtype=torch.float32).reshape(1, -1, 1)
        return kcount(t, cand.sum(-1))

    def _sorted(self, cand):
        s = self.s.masked_fill(~cand, float("-inf"))
        return torch.sort(s, dim=-1, descending=True, stable=True)  # equal values: the lower j first

    def select_topk(self, cand, topk):
        _, idx = self._sorted(cand)
        rank = torch.arange(self.ntk).view(1, 1, 1, -1)
        first = (rank < self.kc(cand, topk).unsqueeze(-1)).expand_as(idx)
        return torch.zeros_like(first).scatter(-1, idx, first) & cand

    def select_cdf(self, cand, cdf):
        p = torch.nan_to_num(torch.softmax(self.s.masked_fill(~cand, float("-inf")), -1), nan=0.0)
        return U.select(p, cand, cdf), p

    def map(self, rule, param, keep_first=0, keep_last=0):
        cand = self.cand(keep_first, keep_last)
        sel = self.select_topk(cand, param) if rule == "topk" else self.select_cdf(cand, param)[0]
        return full_map(sel, cand, self.selfsim)

    def firm(self, cand, topk):
        """-> (firm, strict), bool [B,Hq,nqb].  firm: the k-th and (k+1)-th candidate scores differ by more than the sum of
        their two bounds (rows with kcount = n have no (k+1)-th: firm).  strict: every selected score minus its bound is
        above every other candidate's score plus its bound, which is what makes an fp32 selection equal the fp64 one; the
        CPU tests assert that on these inputs firm implies strict."""
        val, idx = self._sorted(cand)
        bnd = self.bound.gather(-1, idx)
        n = cand.sum(-1).unsqueeze(-1).expand(-1, -1, self.nqb, -1)
        k = self.kc(cand, topk).unsqueeze(-1).expand(-1, -1, self.nqb, -1)
        whole = (k >= n).squeeze(-1)
        ik, ik1 = (k - 1).clamp(min=0), k.clamp(max=self.ntk - 1)
        gap = (val.gather(-1, ik) - val.gather(-1, ik1)).squeeze(-1)
        firm = whole | (gap > (bnd.gather(-1, ik) + bnd.gather(-1, ik1)).squeeze(-1))
        rank = torch.arange(self.ntk).view(1, 1, 1, -1)
        inside, outside = rank < k, (rank >= k) & (rank < n)
        low = torch.where(inside, val - bnd, torch.full_like(val, float("inf"))).amin(-1)
        high = torch.where(outside, val + bnd, torch.full_like(val, float("-inf"))).amax(-1)
        return firm, whole | (low > high)


def rule_of_case(name, dt=torch.float32):
    """The rule on the torch block statistics of a sparge_util case, pooled in `dt`, with the case's simthreshd1."""
    r = U.ref(name)
    pq, sq = U.pool_sim(r.q, 128, dt=dt)
    pk, sk = U.pool_sim(r.k, 64, r.km, dt=dt)
    return Rule(pq, sq, pk, sk, r.sm_scale, r.simthr)
