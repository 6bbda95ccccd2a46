"""drn_amd -- MI355X-native (gfx950) forward/backward hot path of the Dense
Regression Network for video grounding.  Host code is Python; all math runs in
hand-written HIP kernels behind the C-ABI in include/drn_hip.h (libdrn_hip.so).
"""
__version__ = "0.1.0"
from .grounding import Grounder, Hits, Moments, group_by_video, plan_candidate_steps, search  # noqa: E402,F401
from .store import FeatureStore, StoreLoader  # noqa: E402,F401
from .index import SearchIndex  # noqa: E402,F401
from .search_eval import SearchRecall, ShortlistRecall, evaluate_cascade, evaluate_search, evaluate_shortlist, search_batches  # noqa: E402,F401
from .retrieve import (LATE_MAX_TOKENS, SHARDS_MAX, SHORTLIST_DEEP_MAX, Compacted, Pooled, compact_reference, SegmentShortlist, ShardedShortlister, Shortlist, Shortlister, TargetRank,  # noqa: E402,F401
                       candidates_mask, late_rank_reference, late_rerank_reference, late_shortlist_reference, merge_shortlists_reference,
                       pack_allow, pack_allow_reference, plan_segment_blocks, pool_offsets, pool_segments_reference, rank_reference, rank_thresholds_reference, rerank_reference,
                       segment_rank_reference,
                       segment_rerank_reference, segment_shortlist_reference, shard_positions_reference, shortlist_reference,
                       slice_allow_reference)
from .retrieve import (FUSE_MAX_TABLES, FusedShortlister, fuse_scores_reference, fused_rank_reference, fused_shortlist_reference,  # noqa: E402,F401
                       fused_rerank, fused_rerank_reference, rerank_scores_reference, scores_reference, shortlist_scores)
from .retrieve import (RANK_FUSE_MAX_LISTS, RankFusedShortlister, rank_fuse, rank_fuse_rank, rank_fuse_rank_reference,  # noqa: E402,F401
                       rank_fuse_reference)
from .binary import (BINARY_MAX_E, AsymmetricBinaryView, BinaryShortlister, binary_asym_shortlist_reference, binary_dequantize,  # noqa: E402,F401
                     binary_quantize_reference, binary_shortlist_reference, binary_signs)
