"""Paged KV cache: fixed-size blocks from a per-layer device pool.

Sized for MI355X's 288 GB HBM3E: the pool is allocated once up front (no
allocator churn in the decode loop, a requirement for hipGraph capture) and
blocks are handed to sequences from a free list. Layout
[n_blocks, n_kv_heads, block_size, head_dim] keeps one (key, head) row
contiguous (256 B for hd=128 bf16) — the decode kernel reads it as 64 lanes
x 4 B, a perfectly coalesced wave read.

Sliding-window models (release_below): pages whose keys all lie below the
attention window go back to the free list while the sequence lives on. The
block list keeps its logical layout — a released position holds RELEASED
and block_table() emits 0 there, the same valid page the padding points to;
windowed attention never dereferences it.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..models.spec import ModelSpec

# 256-token pages: one decode-attention chunk (DEC_CHUNK) spans exactly one
# page, so the KV stream is 64 KB-sequential per (head, chunk) — measured
# 5.19 -> 5.42/5.54 TB/s at B768/B1536 vs 32-token pages (round 2).
# Allocation granularity coarsens (one page = 256 tokens per sequence),
# which the 288 GB pool absorbs.
BLOCK_SIZE = 256

# block-list marker of a page handed back by release_below()
RELEASED = -1


class PagedKV:
    def __init__(
        self,
        spec: ModelSpec,
        device: torch.device,
        dtype: torch.dtype,
        n_blocks: int,
        block_size: int = BLOCK_SIZE,
        layer_range: Optional[Tuple[int, int]] = None,
        kv_dtype: str = "native",
    ) -> None:
        """kv_dtype: "native" stores the compute dtype; "fp8" stores OCP
        e4m3 bytes (uint8 pool, HALF the KV bytes — the decode kernels read
        fp8 directly; opt-in, reported separately from the bf16 headline)."""
        self.spec = spec
        self.device = device
        self.dtype = dtype
        self.kv_dtype = kv_dtype
        self.block_size = block_size
        self.n_blocks = n_blocks
        lo, hi = layer_range or (0, spec.n_layers)
        self.layer_lo = lo
        store_dtype = torch.uint8 if kv_dtype == "fp8" else dtype
        shape = (n_blocks, spec.n_kv_heads, block_size, spec.head_dim)
        self.k_cache = [
            torch.zeros(shape, device=device, dtype=store_dtype)
            for _ in range(lo, hi)
        ]
        self.v_cache = [
            torch.zeros(shape, device=device, dtype=store_dtype)
            for _ in range(lo, hi)
        ]
        self._free: List[int] = list(range(n_blocks - 1, -1, -1))
        self._seq_blocks: Dict[int, List[int]] = {}
        self._seq_len: Dict[int, int] = {}
        # leading block-list positions already released (release_below)
        self._seq_released: Dict[int, int] = {}
        # Per-(local layer, kv head) fp8 scales: value = float(byte) * scale,
        # byte = e4m3(clamp(x * inv_scale, +-448)). Allocated ONCE and only
        # ever updated in place, so a captured decode graph (which holds the
        # row views below by address) sees new values without recapture.
        # All ones until set_scales(): a never-calibrated fp8 cache stores
        # and reads exactly as with the fixed unit scale.
        self.k_scale = self.v_scale = None
        self.k_inv_scale = self.v_inv_scale = None
        self.scales_source = "unit"
        self._scale_rows: List[Tuple[torch.Tensor, ...]] = []
        if kv_dtype == "fp8":
            ones = lambda: torch.ones(  # noqa: E731
                hi - lo, spec.n_kv_heads, dtype=torch.float32, device=device)
            self.k_scale, self.v_scale = ones(), ones()
            self.k_inv_scale, self.v_inv_scale = ones(), ones()
            self._scale_rows = [
                (self.k_scale[i], self.v_scale[i],
                 self.k_inv_scale[i], self.v_inv_scale[i])
                for i in range(hi - lo)
            ]

    # scratch sequence id (pad rows of graph-bucket batches, engine.py): the
    # one sequence allowed to hold blocks while scales change
    SCRATCH_SEQ = -1

    def layer_scales(self, layer_idx: int):
        """(k_scale, v_scale, k_inv_scale, v_inv_scale) fp32 [n_kv_heads]
        row views for a layer, or None for a non-fp8 cache."""
        if not self._scale_rows:
            return None
        return self._scale_rows[layer_idx - self.layer_lo]

    def check_scales_mutable(self) -> None:
        """Raise unless the scales may change now: an fp8 cache in which no
        sequence but the scratch one holds blocks."""
        if self.kv_dtype != "fp8":
            raise ValueError("KV scales need kv_dtype='fp8'")
        live = [s for s, b in self._seq_blocks.items()
                if b and s != self.SCRATCH_SEQ]
        if live:
            raise RuntimeError(
                f"cannot change KV scales while sequences {live[:4]} hold "
                "cache blocks")

    def set_scales(self, k_scale: torch.Tensor, v_scale: torch.Tensor,
                   source: str = "calibrated") -> None:
        """Install per-(layer, kv head) scales ([n_layers_local, n_kv_heads],
        finite and > 0) in place. Refused while any sequence but the scratch
        one holds blocks: bytes already stored would be read back with the
        wrong scale."""
        self.check_scales_mutable()
        shape = tuple(self.k_scale.shape)
        new = []
        for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
            t = torch.as_tensor(t, dtype=torch.float32)
            if tuple(t.shape) != shape:
                raise ValueError(
                    f"{name} has shape {tuple(t.shape)}, expected {shape} "
                    "([n_layers_local, n_kv_heads])")
            if not bool((torch.isfinite(t) & (t > 0)).all()):
                raise ValueError(f"{name} must be finite and positive")
            new.append(t.to(self.device))
        self.k_scale.copy_(new[0])
        self.v_scale.copy_(new[1])
        # reciprocals once, with torch: no device-side division in kernels
        self.k_inv_scale.copy_(1.0 / self.k_scale)
        self.v_inv_scale.copy_(1.0 / self.v_scale)
        self.scales_source = source

    def layer(self, layer_idx: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.k_cache[layer_idx - self.layer_lo], self.v_cache[layer_idx - self.layer_lo]

    @property
    def free_blocks(self) -> int:
        return len(self._free)

    def new_seq(self, seq_id: int) -> None:
        if seq_id in self._seq_blocks:
            self.free_seq(seq_id)
        self._seq_blocks[seq_id] = []
        self._seq_len[seq_id] = 0
        self._seq_released[seq_id] = 0

    def free_seq(self, seq_id: int) -> None:
        blocks = self._seq_blocks.pop(seq_id, [])
        self._seq_len.pop(seq_id, None)
        # released positions already went back to the free list
        n_rel = self._seq_released.pop(seq_id, 0)
        self._free.extend(reversed(blocks[n_rel:]))

    def release_below(self, seq_id: int, first_live_key: int) -> int:
        """Return to the free list every page of the sequence whose keys
        are all < first_live_key (a page straddling it stays). The logical
        layout is kept: slot_mapping of live positions, seq_len and
        seq_n_blocks do not change. Returns the number of pages released
        by this call."""
        blocks = self._seq_blocks[seq_id]
        n_rel = self._seq_released.get(seq_id, 0)
        upto = min(max(first_live_key, 0) // self.block_size, len(blocks))
        for i in range(n_rel, upto):
            self._free.append(blocks[i])
            blocks[i] = RELEASED
        if upto > n_rel:
            self._seq_released[seq_id] = upto
            return upto - n_rel
        return 0

    def seq_len(self, seq_id: int) -> int:
        return self._seq_len.get(seq_id, 0)

    def seq_n_blocks(self, seq_id: int) -> int:
        """Logical page count (released positions included)."""
        return len(self._seq_blocks.get(seq_id, ()))

    def seq_live_blocks(self, seq_id: int) -> int:
        """Pages the sequence still holds (logical count minus released)."""
        return (len(self._seq_blocks.get(seq_id, ()))
                - self._seq_released.get(seq_id, 0))

    def extend_seq(self, seq_id: int, new_len: int) -> None:
        """Grow a sequence to new_len tokens, allocating blocks as needed.
        All or nothing: a request the pool cannot meet takes no block."""
        blocks = self._seq_blocks[seq_id]
        need = (new_len + self.block_size - 1) // self.block_size
        if need - len(blocks) > len(self._free):
            raise RuntimeError(
                f"KV pool exhausted ({self.n_blocks} blocks of {self.block_size})"
            )
        while len(blocks) < need:
            blocks.append(self._free.pop())
        self._seq_len[seq_id] = new_len

    def slot_mapping(self, seq_id: int, positions: Sequence[int]) -> List[int]:
        blocks = self._seq_blocks[seq_id]
        return [
            blocks[p // self.block_size] * self.block_size + p % self.block_size
            for p in positions
        ]

    def block_table(self, seq_ids: Sequence[int]) -> torch.Tensor:
        """Padded [B, max_blocks] int32 device tensor (0 at released
        positions, like the padding)."""
        tables = [self._seq_blocks[s] for s in seq_ids]
        width = max(1, max(len(t) for t in tables))
        out = torch.zeros(len(tables), width, dtype=torch.int32)
        for i, t in enumerate(tables):
            if t:
                out[i, : len(t)] = torch.tensor(t, dtype=torch.int32)
                n_rel = self._seq_released.get(seq_ids[i], 0)
                if n_rel:
                    out[i, :n_rel] = 0
        return out.to(self.device, non_blocking=True)
