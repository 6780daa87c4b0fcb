"""The calibration of the block-map predictor (include/sageattn_hip.h: sage_attn_tile_mass, sage_block_plan_recall; core.py:
sparge_tune) restated in torch, fp64.  Shared by tests/test_calib.py (CPU) and tests/test_calib_gpu.py.

  tile mass   mass[b,h,i,j] = (1 / c_i) sum over the valid rows r of q-block i, sum over the keys n < N of tile j, of P[r,n];
              P = the softmax over all keys < N; c_i = min(128, M - 128 i).
  recall      recall[b,h,i] = sum of mass[b,h,i,j] over the tiles the map keeps; kept = their number.
  head recall "mean": sum over b, i of c_i recall[b,h,i] / (B M), the mean captured probability per query row; "min": the minimum.
  tune        per head the smallest g / 2^steps, g = 1 .. 2^steps, whose head recall is >= target -- here by trying them all."""
import math

import torch


def _pool(P, M, N):
    """[B,H,M,N'] -> sums over 128 x 64 tiles [B,H,nqb,ntk'] (N' may exceed N: the planted mistake below)"""
    B, H, _, n = P.shape
    nqb, ntk = (M + 127) // 128, (n + 63) // 64
    full = torch.zeros(B, H, nqb * 128, ntk * 64, dtype=P.dtype)
    full[:, :, :M, :n] = P
    return full.view(B, H, nqb, 128, ntk, 64).sum((3, 5))


def valid_rows(M):
    """c_i, fp64 [nqb]"""
    nqb = (M + 127) // 128
    return (M - 128 * torch.arange(nqb)).clamp(max=128).double()


def tile_mass(logits, M, N):
    """logits fp64 [B,Hq,M,N] in natural-log units -> fp64 [B,Hq,ceil(M/128),ceil(N/64)]"""
    assert logits.dtype == torch.float64 and tuple(logits.shape[2:]) == (M, N)
    return _pool(torch.softmax(logits, -1), M, N) / valid_rows(M).view(1, 1, -1, 1)


# ---- two planted mistakes: what a wrong kernel would compute (tests/test_calib.py shows that the GPU tolerance sees them)
def tile_mass_counts_padding(logits, M, N):
    """the keys >= N of the last tile take part: the kernel stages row N - 1 again for them, so they score like the last key"""
    ntk = (N + 63) // 64
    padded = torch.cat([logits, logits[..., N - 1:].expand(*logits.shape[:3], ntk * 64 - N)], -1)
    return _pool(torch.softmax(padded, -1), M, N) / valid_rows(M).view(1, 1, -1, 1)


def tile_mass_weights_128(logits, M, N):
    """a ragged q-block divided by 128 instead of by its valid rows"""
    return _pool(torch.softmax(logits, -1), M, N) / 128.0


def recall(bm, mass):
    """bm bool [B|1,Hq|1,nqb,ntk], mass [B,Hq,nqb,ntk] -> (recall [B,Hq,nqb] in mass's dtype, kept int64 [B,Hq,nqb])"""
    bm = bm.expand(mass.shape)
    return (mass * bm).sum(-1), bm.sum(-1)


def head_recall(rec, M, reduce):
    """rec [B,Hq,nqb] -> [Hq]"""
    if reduce == "min":
        return rec.amin((0, 2))
    return (rec * valid_rows(M).to(rec.dtype).view(1, 1, -1)).sum((0, 2)) / (rec.shape[0] * M)


def tune(head_recall_at, steps, target):
    """Brute force over the whole grid.  head_recall_at(g) -> [Hq] head recall at the parameter g / 2^steps.
    -> (param, met, recall, recall_below), each [Hq], as sparge_tune defines them; and the [2^steps, Hq] table of recalls."""
    n = 1 << steps
    table = torch.stack([head_recall_at(g) for g in range(1, n + 1)])  # row g - 1
    ok = table >= target
    met = ok[-1].clone()
    first = torch.where(ok.any(0), ok.float().argmax(0), torch.full_like(ok[0], n - 1, dtype=torch.long))  # row of param
    first = torch.where(met, first, torch.full_like(first, n - 1))
    param = (first + 1).to(table.dtype) / n
    rec = table.gather(0, first.view(1, -1)).squeeze(0)
    below = table.gather(0, (first - 1).clamp(min=0).view(1, -1)).squeeze(0)
    below = torch.where(first > 0, below, torch.full_like(below, -math.inf))
    return param, met, rec, below, table
