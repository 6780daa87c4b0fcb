"""Block-map helpers shared by the block-sparse tests: 128-row q-blocks x 64-key tiles."""
import torch


def make_map(B, H, M, N, density, seed):
    """Seeded random bool map [B, H, ceil(M/128), ceil(N/64)] with every q-block keeping at least one tile."""
    g = torch.Generator().manual_seed(seed)
    nqb, ntk = (M + 127) // 128, (N + 63) // 64
    bm = torch.rand(B, H, nqb, ntk, generator=g) < density
    first = torch.randint(0, ntk, (B, H, nqb, 1), generator=g)
    return bm | (~bm.any(-1, keepdim=True) & (torch.arange(ntk).view(1, 1, 1, ntk) == first))


def expand_map(bm, M, N):
    """The block map as an element mask [B, H, M, N]."""
    return bm.repeat_interleave(128, dim=2)[:, :, :M].repeat_interleave(64, dim=3)[..., :N]


def gather_block(tiles_on, N):
    """Key indices (ascending, cut at N) of the active tiles of one list row (bool [ceil(N/64)])."""
    idx = torch.nonzero(tiles_on).flatten()
    cols = (idx.view(-1, 1) * 64 + torch.arange(64).view(1, 64)).flatten()
    return cols[cols < N]
