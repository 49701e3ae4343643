"""Launch-selection options of the hot path: ONE object, read at call time.

Every alternative launch sequence the path can take (a fused kernel against the launches it replaces, the gradient side
stream, the flat-layout fast paths) is selected by a field of ``opts``.  The fields are initialised once from ``FD_*``
environment variables (so ``tools/ablation.sh`` keeps working) and can be flipped afterwards -- by tests, without
re-importing anything:

    from se3_diffusion_amd import options
    with options.override(fused_edge=False, grad_stream=False):
        ...

Both settings of every field are covered by a parity test (tests/test_switches.py, tests/test_parity_full.py's exact-fp32
mode, tests/test_seq_attn.py).  ``FD_GEMM_EXACT_F32`` is not here: it is state of the loaded library
(``hip.FdLib.set_exact_f32``), because the C side consults it too.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os


def _flag(name, default):
    return os.environ.get(name, "1" if default else "0") not in ("", "0")


def _int(name, default):
    return int(os.environ.get(name, str(default)))


def _opt(env, default):
    """A field of Options, declared once: its FD_* environment variable (read by Options.from_env) and its default."""
    return dataclasses.field(default=default, metadata={"env": env})


@dataclasses.dataclass
class Options:
    # -- streams
    grad_stream: bool = _opt("FD_GRAD_STREAM", True)                    # weight gradients on a second HIP stream beside the dX chain (ops.side)
    grad_stream_max_rows: int = _opt("FD_GRAD_STREAM_ROWS", 1 << 40)    # row count above which a launch stays on the main stream
    side_stream_priority: int = _opt("FD_SIDE_PRIORITY", 0)             # HIP priority of that stream (lower = higher; clamped to the device's range)
    # -- pair level
    fused_edge: bool = _opt("FD_EDGE_FUSED", True)                      # fd_edge_mlp (whole edge-transition chain per pair row) vs the GEMM sequence
    fused_embed: bool = _opt("FD_EMBED_FUSED", True)                    # fd_edge_embed (features generated in registers) vs fd_edge_feats + GEMMs
    fused_embed_bwd: bool = _opt("FD_EMBED_BWD_FUSED", True)            # the edge embedder's dX chain in one launch (fd_edge_embed_bwd)
    grouped_pair_dw: bool = _opt("FD_PAIR_DW", True)                    # the edge transition's pair-row weight gradients in one grouped launch
    pair_dw_blocks: int = _opt("FD_PAIR_DW_BLOCKS", 160)                # blocks of fd_pair_dw when it runs beside the main stream (0 = 256)
    edge_blocks: int = _opt("FD_EDGE_BLOCKS", 0)                        # persistent blocks of the fused edge kernels (0 = fill the CUs: 512 / 256)
    edge_shape: int = _opt("FD_EDGE_SHAPE", 0)                          # 0 = by size, 4 = 4-wave blocks (two per CU), 8 = 8-wave blocks (one per CU),
                                                                        # 2 = two waves per 16-row group (inference forward launches only; the others keep the size rule)
    edge_pair: bool = _opt("FD_EDGE_PAIR", True)                        # sampling -- an edge transition of at most 16,384 pair rows (a lone N <= 128 backbone:
                                                                        # one 16-row group per SIMD) on the column-split kernel, two waves per group (fd_edge_mlp_pair.hip)
    edge_dynamic_tiles: bool = _opt("FD_EDGE_DYN_TILES", True)          # a fused edge launch with more tiles than blocks hands them out dynamically
    packed_gates: bool = _opt("FD_PACKED_GATES", True)                  # the fused edge EMBEDDER's backward gates on packed sign bits instead of reading h1 / h2
                                                                        # (the edge transition's always does: its h2 save carries the residual z)
    fused_ln_bwd: bool = _opt("FD_EDGE_LN_BWD", True)                   # the edge transition's LayerNorm backward (and the IPA term dz += dzb W40 of
                                                                        # the block behind it) as the prologue of its fused backward kernel
    zb_from_edge: bool = _opt("FD_ZB_FUSED", True)                      # the next IPA block's pair projection zb as a 4th layer of fd_edge_mlp
    fold_node_terms: bool = _opt("FD_FOLD_NODE_TERMS", True)            # sampling -- per-residue terms of an edge transition as one GEMM
    # -- IPA
    fused_ipa_attn: bool = _opt("FD_IPA_ATTN_FUSED", True)              # logits + softmax + o_pair of a query row in one launch
    flash_ipa: bool = _opt("FD_IPA_FLASH", True)                        # q k^T, logits, softmax, a v, a v_pts, o_pt and o_pair of a block in ONE launch
                                                                        # (fd_ipa_flash_fwd: the probabilities never reach HBM in inference) ...
    flash_ipa_min_tiles: int = _opt("FD_IPA_FLASH_MIN_TILES", 80)       # ... from this many 16-row query tiles (B * ceil(N / 16)) up: a lone
                                                                        # backbone has too few tiles to fill the CUs and keeps the launch sequence (measured: 95 tiles
                                                                        # 151 against 180 us with the probabilities written, 75 tiles 192 against 195, 56 tiles 210 against 171)
    flash_ipa_bwd: bool = _opt("FD_IPA_FLASH_BWD", True)                # the query side of IPA's attention backward in one launch (fd_ipa_flash_bwd: no dA
                                                                        # in HBM) instead of two batched GEMMs + fd_ipa_attn_bwd's per-row kernel ...
    flash_ipa_keys: bool = _opt("FD_IPA_FLASH_KEYS", True)              # ... and its key side (dV, dv_pts, dK, dk_pts) in one launch (fd_ipa_flash_bwd_keys: A and dL
                                                                        # read once) instead of three batched GEMMs + fd_ipa_kpts_bwd, where the query side runs fused ...
    flash_ipa_keys_max_n: int = _opt("FD_IPA_FLASH_KEYS_MAX_N", 384)    # ... up to this N (four key tiles of a head per block, the query operands through
                                                                        # LDS once per block: B=30 x N=128 78 against 102 us, B=12 x N=200 97 against 119, B=7 x N=256 82 against
                                                                        # 109; B=8 x N=512 248 against 225, B=1 x N=512 138 against 102: long chains keep the batched GEMMs)
    flash_ipa_bwd_min_tiles: int = _opt("FD_IPA_FLASH_BWD_MIN_TILES", 128)  # ... from this many query tiles up (8 heads per block only: 112 tiles
                                                                        # 195 against 199 us, 95 tiles 224 against 207)
    flash_ipa_split_min_n: int = _opt("FD_IPA_FLASH_SPLIT_MIN_N", 384)  # inference below flash_ipa_min_tiles -- from this N up the KEYS of a query tile are
                                                                        # split over 4 blocks + a merge launch (fd_ipa_flash_fwd_split: 86 against 112 us at N=512 B=1; 55
                                                                        # against 49 at N=256, 42 against 39 at N=128: the launch sequence stays there)
    flash_ipa_splits: int = _opt("FD_IPA_FLASH_SPLITS", 4)              # ... key splits of that form
    flash_ipa_hpb: int = _opt("FD_IPA_FLASH_HPB", 0)                    # heads per block of that kernel (0 = by size, 8 / 4 / 2)
    proj_merge: bool = _opt("FD_PROJ_MERGE", True)                      # IPA's four projections of s as one GEMM over back-to-back weights
    # -- node level
    fused_seq_attn: bool = _opt("FD_SEQ_ATTN_FUSED", True)              # sequence-transformer attention in one launch ...
    seq_attn_min_rows: int = _opt("FD_SEQ_ATTN_MIN_ROWS", 1024)         # ... from this many residue rows up
    fused_seq_attn_bwd: bool = _opt("FD_SEQ_ATTN_BWD_FUSED", True)      # its backward (dQ, dK, dV from the saved probabilities and output) in one launch
                                                                        # (fd_seq_attn_bwd) instead of four batched GEMMs + the row-softmax backward
    grouped_node_dw: bool = _opt("FD_NODE_DW", True)                    # the node-level weight gradients of a trunk block in one grouped launch
    defer_node_dw: bool = _opt("FD_DEFER_NODE_DW", True)                # ... launched behind the NEXT edge transition's fused backward (beside that block's
                                                                        # node-level phase) instead of at the end of its own block (in front of that full-chip kernel)
    node_dw_blocks: int = _opt("FD_NODE_DW_BLOCKS", 0)                  # its persistent blocks (0 = 512: two per CU)
    weight_planes: bool = _opt("FD_WEIGHT_PLANES", True)                # training -- the flat parameter buffer split into its three bf16 planes once per step
                                                                        # (fd_split_planes); the node-level GEMMs then read the weight operand pre-split (fd_gemm tiles 12-14)
    ln_fold: bool = _opt("FD_LN_FOLD", True)                            # sampling -- the sequence transformer's LayerNorms inside the GEMM launches that
                                                                        # consume them (fd_ln_gemm) instead of launches of their own
    sampler_device_steps: bool = _opt("FD_SAMPLER_DEVICE_STEPS", True)  # sampling -- the captured step takes t, the step's scalars and its normal draws
                                                                        # from device arrays indexed by a device counter (fd_sample_advance) instead of three launches per step
    embed_first_padded: bool = _opt("FD_EMBED_FIRST_PADDED", True)      # sampling -- the per-residue features at a row stride of 72 (fd_node_feats_ld) so that the
                                                                        # embedders' first layers (K = 65 / 33) run on the latency GEMM; p | q of the edge embedder as ONE product
    merge_skip_embed: bool = _opt("FD_MERGE_SKIP", True)                # sampling -- the skip_embed products of all trunk blocks as ONE GEMM per forward
    # -- backward bookkeeping
    zero_arena: bool = _opt("FD_ZERO_ARENA", True)                      # one memset for every zero-initialised accumulator of a backward pass
    dx_splitk: bool = _opt("FD_DX_SPLITK", True)                        # accumulating dX GEMMs with a long reduction split over K (atomics)

    @classmethod
    def from_env(cls):
        """Every field from its environment variable: a bool default reads a flag ("" and "0" are off), an int default an integer."""
        return cls(**{f.name: (_flag if isinstance(f.default, bool) else _int)(f.metadata["env"], f.default)
                      for f in dataclasses.fields(cls)})


opts = Options.from_env()


@contextlib.contextmanager
def override(**kw):
    """Temporarily set fields of ``opts`` (unknown names raise)."""
    was = {}
    for k, v in kw.items():
        if not hasattr(opts, k):
            raise AttributeError(f"unknown option {k!r}")
        was[k] = getattr(opts, k)
        setattr(opts, k, v)
    try:
        yield opts
    finally:
        for k, v in was.items():
            setattr(opts, k, v)
