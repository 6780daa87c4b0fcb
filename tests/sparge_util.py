"""The block-map predictor's rule (include/sageattn_hip.h, sage_block_pool_sim / sage_block_select_cdf) restated in torch,
in any float dtype -- the tests use fp64 -- and the clustered inputs its tests run on.  Shared by tests/test_sparge.py (CPU)
and tests/test_sparge_gpu.py.

Inputs: per (b, h, block) a centre ~ N(0, 2^2 I_D), tokens = centre + N(0, I); every 4th Q block and every 5th K block has
no centre (pure noise: not self-similar); K gets +3.0 on every channel, so that a predictor that ignores the smoothing mean
sees every K block as self-similar.  Seeded, generated on the CPU."""
import functools

import torch

DELTA = 2.0 ** -8      # slack of the selection properties in units of softmax mass
CDFS = (0.5, 0.9, 0.98)

# name -> D, M, N, Hq, Hk, B, dtype.  The smallest shapes that reach every path:
#   c1   ragged blocks on both sides, GQA
#   c2   71 key tiles: more than one 64-lane step of the selection's wave
#   c3   a one-row last q-block, no ragged key tile;  c3bf: the same in bf16
CASES = {
    "c1": (64, 128 * 3 + 50, 64 * 9 + 37, 4, 2, 2, torch.float16),
    "c2": (128, 256, 64 * 70 + 5, 4, 2, 2, torch.float16),
    "c3": (128, 128 * 5 + 1, 64 * 21, 2, 2, 2, torch.float16),
    "c3bf": (128, 128 * 5 + 1, 64 * 21, 2, 2, 2, torch.bfloat16),
}


def _clustered(B, H, n, D, blk, noise_every, offset, gen):
    nb = (n + blk - 1) // blk
    c = torch.randn(B, H, nb, 1, D, generator=gen) * 2.0
    noisy = (torch.arange(nb) % noise_every == noise_every - 1).view(1, 1, nb, 1, 1)
    c = torch.where(noisy, torch.zeros_like(c), c)
    x = c + torch.randn(B, H, nb, blk, D, generator=gen)
    return x.reshape(B, H, nb * blk, D)[:, :, :n] + offset


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> q [B,Hq,M,D], k [B,Hk,N,D] (CPU, the case's dtype).  Do not modify: shared."""
    D, M, N, Hq, Hk, B, dtype = CASES[name]
    g = torch.Generator().manual_seed(D + M + N)
    q = _clustered(B, Hq, M, D, 128, 4, 0.0, g)
    k = _clustered(B, Hk, N, D, 64, 5, 3.0, g)
    return q.to(dtype), k.to(dtype)


def pool_sim(x, blk, mean=None, dt=torch.float64):
    """pooled [B,H,nb,D], sim [B,H,nb] of x - mean in dtype dt."""
    B, H, n, D = x.shape
    nb = (n + blk - 1) // blk
    x = x.to(dt)
    if mean is not None:
        x = x - mean.to(dt).unsqueeze(2)
    x = torch.cat([x, torch.zeros(B, H, nb * blk - n, D, dtype=dt)], 2).view(B, H, nb, blk, D)
    cnt = torch.full((nb,), blk, dtype=dt)
    cnt[-1] = n - (nb - 1) * blk
    cnt = cnt.view(1, 1, nb)
    pooled = x.sum(3) / cnt.unsqueeze(-1)
    nrm = x.norm(dim=-1, keepdim=True)
    unit = torch.where(nrm > 0, x / nrm, torch.zeros_like(x))  # padded rows are zero rows: they contribute nothing
    s = unit.sum(3)
    return pooled, (s * s).sum(-1) / (cnt * cnt)


def sim_explicit(x, blk, mean=None):
    """sim as its definition: the mean of the c x c cosine matrix of every block (fp64)."""
    B, H, n, D = x.shape
    x = x.double()
    if mean is not None:
        x = x - mean.double().unsqueeze(2)
    out = []
    for r0 in range(0, n, blk):
        rows = x[:, :, r0:r0 + blk]
        nrm = rows.norm(dim=-1, keepdim=True)
        unit = torch.where(nrm > 0, rows / nrm, torch.zeros_like(rows))
        out.append((unit @ unit.transpose(-1, -2)).mean((-1, -2)))
    return torch.stack(out, -1)


def probs(pq, sq, pk, sk, sm_scale, simthr):
    """-> p [B,Hq,nqb,ntk] (softmax over the eligible key blocks, 0 elsewhere), elig [B,Hq,1,ntk], selfsim [B,Hq,nqb,1].
    simthr: float or [Hq]."""
    g = pq.shape[1] // pk.shape[1]
    pk, sk = pk.repeat_interleave(g, 1), sk.repeat_interleave(g, 1)
    thr = torch.as_tensor(simthr, dtype=sk.dtype).reshape(1, -1, 1)
    s = (pq @ pk.transpose(-1, -2)) * sm_scale
    elig = (sk > thr).unsqueeze(2)
    p = torch.softmax(s.masked_fill(~elig, float("-inf")), -1)
    return torch.nan_to_num(p, nan=0.0), elig, (sq > thr).unsqueeze(-1)


def select(p, elig, cdf):
    """The shortest prefix of the eligible blocks in descending p (ties: lower index) whose sum is >= cdf * sum(p).
    cdf: float or [Hq]."""
    cdf = torch.as_tensor(cdf, dtype=p.dtype).reshape(1, -1, 1, 1)
    val, idx = torch.sort(p, dim=-1, descending=True, stable=True)
    cum = torch.cumsum(val, -1)
    first = (cum >= cdf * cum[..., -1:]).float().argmax(-1, keepdim=True)
    rank = torch.arange(p.shape[-1]).view(1, 1, 1, -1)
    sel = torch.zeros_like(p, dtype=torch.bool).scatter(-1, idx, (rank <= first).expand_as(p)) & elig
    return torch.where(cdf >= 1, elig.expand_as(sel), sel)


def full_map(sel, elig, selfsim):
    """Tile (i, j) is on if j is selected, or j is not eligible, or i is not self-similar."""
    return sel | ~elig | ~selfsim


class Ref:
    """Everything the tests need of one case, in fp64, for a given smoothing mean."""

    def __init__(self, name, km=None):
        self.name = name
        self.D, self.M, self.N, self.Hq, self.Hk, self.B, self.dtype = CASES[name]
        self.q, self.k = inputs(name)
        self.km = self.k.double().mean(2).to(self.dtype) if km is None else km
        self.sm_scale = self.D ** -0.5
        self.pq, self.sq = pool_sim(self.q, 128)
        self.pk, self.sk = pool_sim(self.k, 64, self.km)
        # simthreshd1: the midpoint of the largest gap in the sorted sim values, so that no eligibility decision can depend
        # on rounding (the tests assert the gap is >= 0.1)
        allsim = torch.cat([self.sq.flatten(), self.sk.flatten()]).sort().values
        gaps = allsim[1:] - allsim[:-1]
        i = int(gaps.argmax())
        self.gap = (float(allsim[i]), float(allsim[i + 1]))
        self.simthr = 0.5 * (self.gap[0] + self.gap[1])
        self.p, self.elig, self.selfsim = probs(self.pq, self.sq, self.pk, self.sk, self.sm_scale, self.simthr)
        self.live = self.selfsim.squeeze(-1) & self.elig.any(-1)  # rows in which a selection takes place

    def map(self, cdf):
        return full_map(select(self.p, self.elig, cdf), self.elig, self.selfsim)

    def marginal(self, cdf):
        """bool per list row: the selection at cdf - DELTA differs from the one at cdf + DELTA."""
        return ((select(self.p, self.elig, cdf - DELTA) != select(self.p, self.elig, cdf + DELTA)).any(-1)
                & self.selfsim.squeeze(-1))


@functools.lru_cache(maxsize=None)
def ref(name):
    return Ref(name)
