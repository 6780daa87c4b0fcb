"""The rule of the paged KV cache (include/sageattn_hip_paged.h) restated for the tests: where a logical 64-key tile lives, the
padded tensors a block table describes, and pools with a poison page.

No table the tests build holds an id outside [0, P]: entries a sequence does not use name the POISON page, whose fp16 / bf16
rows are NaN -- a wrong read shows as wrong bits, never as a fault."""
import torch

import kvcache_util as KU

PAGE_SIZES = (64, 128, 256)


# ---- host arithmetic -------------------------------------------------------------------------------------------------------
def tiles_per_page(page_size):
    assert page_size in PAGE_SIZES
    return page_size // 64


def tile_slot(t, page_size):
    """logical 64-key tile t -> (index into the table row, tile inside that page)"""
    tpp = tiles_per_page(page_size)
    return t // tpp, t % tpp


def tile_home(row, t, page_size):
    """logical tile t of the sequence whose table row is ``row`` (a list) -> (page id, tile inside the page)"""
    i, ti = tile_slot(t, page_size)
    return row[i], ti


def pages_needed(length, page_size):
    return (max(int(length), 0) + page_size - 1) // page_size


def touched_k_homes(row, start, length, N, page_size):
    """[(page, tile in page)] of the K tiles an append touches, in logical order"""
    return [tile_home(row, t, page_size) for t in KU.touched_tiles(start, length, N)]


def touched_v_homes(row, start, length, N, D, page_size):
    """... of the 64-token V^T blocks it may write: at head_dim 64 a workgroup holds the two blocks of a unit, which with
    64-key pages are two lookups"""
    return [tile_home(row, t, page_size) for t in KU.touched_v_blocks(start, length, N, D)]


# ---- pools and tables ------------------------------------------------------------------------------------------------------
def hnd_pool(pool, layout):
    """the [P,H,page_size,D] view of a K / V / INT8 pool, or the [P,H,D,page_size] view of the pool of V^T images"""
    return pool if layout == "HND" else pool.transpose(1, 2)


def make_pools(P, Hk, page_size, D, layout, dtype, device, seed=0):
    """k_pool, v_pool with P pages of random rows and one more, the poison page (id P): all NaN"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    shape = (P + 1, Hk, page_size, D) if layout == "HND" else (P + 1, page_size, Hk, D)
    k = (torch.randn(shape, generator=g) * 1.5 + 0.3).to(dtype).to(device)
    v = torch.randn(shape, generator=g).to(dtype).to(device)
    k[P] = float("nan")
    v[P] = float("nan")
    return k, v, P


def make_table(lens_max, max_pages, page_size, P, poison, seed=0, reverse_row=None):
    """int32 [B, max_pages] (CPU): row b names pages_needed(lens_max[b]) distinct pages, a random draw without replacement
    over all rows (so the rows are non-monotone; ``reverse_row`` is put in descending page order), then the poison page"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    perm = torch.randperm(P, generator=g).tolist()
    table = torch.full((len(lens_max), max_pages), poison, dtype=torch.int32)
    for b, n in enumerate(lens_max):
        need = pages_needed(n, page_size)
        assert need <= max_pages and need <= len(perm)
        mine, perm = perm[:need], perm[need:]
        if b == reverse_row:
            mine = sorted(mine, reverse=True)
        table[b, :need] = torch.tensor(mine, dtype=torch.int32)
    return table


def gather(pool, table, layout):
    """the padded tensor of the rule: [B,H,N,D] (NHD: [B,N,H,D]) made of each row's pages in table order, N = max_pages *
    page_size -- every entry is followed, the poison page included"""
    x = pool[table.long().to(pool.device)]
    B, mp = table.shape
    if layout == "HND":
        x = x.permute(0, 2, 1, 3, 4)
        return x.reshape(B, x.size(1), mp * x.size(3), x.size(4)).contiguous()
    return x.reshape(B, mp * x.size(2), x.size(3), x.size(4)).contiguous()


def poison_tails(k_pool, v_pool, table, lens, layout):
    """NaN into the rows >= len_b of each sequence's last page in the fp16 / bf16 pools"""
    page_size = hnd_pool(k_pool, layout).size(2)
    for b, n in enumerate(lens):
        if n == 0 or n % page_size == 0:
            continue
        page = int(table[b, (n - 1) // page_size])
        for pool in (k_pool, v_pool):
            hnd_pool(pool, layout)[page, :, n % page_size:] = float("nan")


# ---- the paged state against the contiguous cache --------------------------------------------------------------------------
def valid_tile_views(cache, ref, table, lens):
    """yields (what, paged bytes, reference bytes) for every valid logical tile: INT8 rows < len_b, the tile's scales, and for
    FP8 P.V its V^T block"""
    layout = cache.tensor_layout
    ps, g = cache.page_size, KU.gpb(cache)
    k8p, k8r = hnd_pool(cache.k8, layout), KU.hnd(ref.k8, layout)
    fp8 = cache.pv == "fp8"
    if fp8:
        v8p, v8r = hnd_pool(cache.v8.view(torch.uint8), layout), KU.hnd(ref.v8.view(torch.uint8), layout)
    for b, n in enumerate(lens):
        for t in range((n + 63) // 64):
            page, ti = tile_home(table[b].tolist(), t, ps)
            rows = min(64, n - 64 * t)
            yield ("k8", b, t), k8p[page, :, 64 * ti:64 * ti + rows], k8r[b, :, 64 * t:64 * t + rows]
            yield ("k_scale", b, t), cache.k_scale[page, :, g * ti:g * ti + g], ref.k_scale[b, :, g * t:g * t + g]
            if fp8:
                yield ("v8", b, t), v8p[page, :, :, 64 * ti:64 * ti + 64], v8r[b, :, :, 64 * t:64 * t + 64]


def assert_state_equals_ref(cache, ref, table, lens):
    assert torch.equal(cache.km.view(torch.int16), ref.km.view(torch.int16)), "km"
    if cache.pv == "fp8":
        # (of the batches that have keys: the length-aware pre-pass never writes the V scale of a batch without any -- the
        #  reference's own value there is whatever its allocation held, and no kernel reads it)
        has = torch.tensor([n > 0 for n in lens], device=cache.v_scale.device)
        assert torch.equal(cache.v_scale.view(torch.int32)[has], ref.v_scale.view(torch.int32)[has]), "v_scale"
        assert torch.equal(cache.v_coef.view(torch.int32)[has], ref.v_coef.view(torch.int32)[has]), "v_coef"
    for what, got, want in valid_tile_views(cache, ref, table, lens):
        assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), what


def touched_masks(cache, table, spans):
    """bool masks (k8, k_scale, v8 or None), shaped as the HND views of the pools: True where some append of ``spans`` -- a
    list of (start lens, lens) per call -- may have written.  INT8 rows >= len_b of a touched tile are NOT written."""
    layout, ps, g = cache.tensor_layout, cache.page_size, KU.gpb(cache)
    N = table.shape[1] * ps
    D = cache.k.size(-1)
    mk = torch.zeros(hnd_pool(cache.k8, layout).shape, dtype=torch.bool)
    ms = torch.zeros(cache.k_scale.shape, dtype=torch.bool)
    mv = torch.zeros(hnd_pool(cache.v8, layout).shape, dtype=torch.bool) if cache.pv == "fp8" else None
    for starts, lens in spans:
        for b, (s, n) in enumerate(zip(starts, lens)):
            row = table[b].tolist()
            for t in KU.touched_tiles(s, n, N):
                page, ti = tile_home(row, t, ps)
                mk[page, :, 64 * ti:64 * ti + min(64, n - 64 * t)] = True
                ms[page, :, g * ti:g * ti + g] = True
            if mv is not None:
                for t in KU.touched_v_blocks(s, n, N, D):
                    page, ti = tile_home(row, t, ps)
                    mv[page, :, :, 64 * ti:64 * ti + 64] = True
    return mk, ms, mv
