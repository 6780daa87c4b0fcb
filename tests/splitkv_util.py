"""The rule of split-KV attention (include/sageattn_hip.h, split-KV attention) restated in torch for the tests: the key-tile
range of every (length, split), the column-range block maps under which ``sageattn_block_sparse`` is the oracle of a split's
partial result, and the fp64 merge of those partials through tests/seqpar_ref.py.  CPU only; nothing of the library."""
import torch

from seqpar_ref import merge_ref, ulp

SPLITKV_MAX = 16


def clamp_len(n, N):
    return min(max(int(n), 0), N)


def split_range(length, S, s):
    """(t0, t1): the key tiles of split ``s`` of a batch with ``length`` valid keys under ``S`` splits; t0 >= t1: empty"""
    ntk = (length + 63) // 64
    tps = -(-ntk // S)
    t0 = s * tps
    return t0, max(t0, min(t0 + tps, ntk))


def nonempty_splits(length, S):
    """the number of non-empty splits: ceil(ntk / tps), 0 without keys -- what the merge kernel derives"""
    ntk = (length + 63) // 64
    tps = -(-ntk // S)
    return -(-ntk // tps) if tps else 0


def range_map(lens, N, M, Hq, S, s):
    """bool [B, Hq, ceil(M/128), ceil(N/64)]: on in exactly the tile columns of split ``s`` of every batch, for every q-block.
    ``lens``: the clamped length of every batch."""
    nqb, ntk = (M + 127) // 128, (N + 63) // 64
    bm = torch.zeros(len(lens), Hq, nqb, ntk, dtype=torch.bool)
    for b, n in enumerate(lens):
        t0, t1 = split_range(n, S, s)
        bm[b, :, :, t0:t1] = True
    return bm


def merged_reference(o_parts, lse_parts, dtype, o_got):
    """fp64 merge of the oracle partials (o_s [B,Hq,M,D] in ``dtype``, lse_s [B,Hq,M] natural log with the smoothing correction
    in it; a split that is empty for a batch has lse = -inf there) -> (MergeRef on rows [B*Hq*M], o_extra [rows, D]).
    ``o_got`` [rows, D]: the result under test, for the binade of its final rounding only.

    o_extra holds the two terms by which the kernel's result may differ beyond check_merge's own bound.  With x_s the fp32
    partial the kernel merges, y_s = round(x_s) the oracle's, w_s the weights and z the kernel's fp32 merged value:
      * every |x_s - y_s| <= ulp(y_s) / 2 (x_s and y_s share a binade, or y_s is the power of two above it), so the merged
        oracle carries at most sum_s w_s * ulp(y_s) / 2 that the merge of the fp32 partials does not;
      * the one rounding to ``dtype`` moves z by at most half an ulp OF THE BINADE OF z, which is that of the rounded result
        (or the one below it); check_merge charges ulp(ref.o) / 2, the binade of the reference.  Where the result lies a
        binade above the reference -- the reference just below a power of two, z just above it -- the ulp doubles: the term
        (ulp(max(|o|, |ref.o|)) - ulp(ref.o)) / 2, zero everywhere else, as km_tolerance of seqpar_ref.py takes its half ulp
        "at the larger of the two magnitudes".
    Neither term is fitted to a result."""
    D = o_parts[0].shape[-1]
    os_ = [o.detach().cpu().reshape(-1, D) for o in o_parts]
    ls = [l.detach().cpu().reshape(-1) for l in lse_parts]
    ref = merge_ref(os_, ls)
    l = torch.stack([t.double() for t in ls])
    empty = torch.isinf(l) & (l < 0)
    mx = l.amax(0)
    some = ~torch.isinf(mx)
    e = torch.where(empty | ~some, torch.zeros_like(l), torch.exp(l - torch.where(some, mx, torch.zeros_like(mx))))
    w = e / torch.where(some, e.sum(0), torch.ones_like(mx))
    o = torch.stack([t.double() for t in os_])
    half = torch.where(empty.unsqueeze(-1), torch.zeros_like(o), 0.5 * ulp(o, dtype))
    big = torch.maximum(ref.o.abs(), o_got.detach().cpu().double().abs())
    edge = 0.5 * (ulp(big, dtype) - ulp(ref.o, dtype))
    return ref, (w.unsqueeze(-1) * half).sum(0) + edge
