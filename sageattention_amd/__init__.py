"""sageattention_amd -- MI355X (gfx950) native drop-in for the SageAttention quantized attention operator.

Exports the names the reference package exports (sageattention/__init__.py:25-95): ``sageattn`` plus the
``sageattn_qk_int8_*`` entry points that diffusers imports by name."""
from .core import (sageattn, sageattn_qk_int8_pv_fp16_cuda, sageattn_qk_int8_pv_fp16_triton,
                   sageattn_qk_int8_pv_fp8_cuda, sageattn_qk_int8_pv_fp8_cuda_sm90, sageattn_varlen,
                   sageattn_block_sparse, block_sparse_plan, BlockSparsePlan, sageattn_sparge, sparge_plan,
                   sageattn_tile_mass, plan_recall, sparge_tune, SpargeTuning, sageattn_kvlen,
                   sageattn_tile_mass_kvlen, plan_recall_kvlen, sparge_tune_kvlen, sageattn_splitkv, splitkv_num_splits,
                   sageattn_splitkv_causal)
from . import quant, _qattn, _fused  # noqa: F401
from .ring import ring_sageattn  # noqa: F401  (sequence parallel, RCCL send/recv)
from .ulysses import ulysses_sageattn  # noqa: F401  (head parallel, RCCL all-to-all)
from .kvcache import SageKVCache, sageattn_splitkv_cached  # a persistent quantized KV cache for the split-KV operators
from .paged import SagePagedKVCache, sageattn_splitkv_paged  # ... kept in pages of one pool, addressed through a block table
from .paged_rows import SagePagedRowCache  # ... that owns every pool and takes the step's new rows: no fp16 K pool
from .prefix import sageattn_splitkv_paged_prefix  # ... with a prefix the sequences share, stored and read once

__all__ = ["sageattn", "sageattn_qk_int8_pv_fp16_cuda", "sageattn_qk_int8_pv_fp16_triton",
           "sageattn_qk_int8_pv_fp8_cuda", "sageattn_qk_int8_pv_fp8_cuda_sm90", "sageattn_varlen", "ring_sageattn",
           "ulysses_sageattn", "sageattn_block_sparse", "block_sparse_plan", "BlockSparsePlan", "sageattn_sparge",
           "sparge_plan", "sageattn_tile_mass", "plan_recall", "sparge_tune", "SpargeTuning", "sageattn_kvlen",
           "sageattn_tile_mass_kvlen", "plan_recall_kvlen", "sparge_tune_kvlen", "sageattn_splitkv", "splitkv_num_splits",
           "sageattn_splitkv_causal", "SageKVCache", "sageattn_splitkv_cached",
           "SagePagedKVCache", "sageattn_splitkv_paged", "SagePagedRowCache", "sageattn_splitkv_paged_prefix"]
__version__ = "0.2.0"
