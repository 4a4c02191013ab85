"""The decode step's device inputs and its hipGraph-captured replay.

One decode step reads four device tensors, one row per sequence:

    ids        int64 [B]     token fed to the step (the last one sampled)
    positions  int32 [B]     its position, i.e. tokens already in the cache
    seq_lens   int32 [B]     positions + 1
    block_table int32 [B, W] KV pages of each sequence

`DecodeState` is their only writer. `load()` rebuilds them from host
lists, `advance()` bumps them in place with device ops, `logits()` runs the
step. The engine's serving step and its benchmark step are both callers of
those three and hold no copy of the inputs themselves.

With `DecodeGraphs` the four tensors are views of its static buffers
[max_batch(, width)], whose storage never moves: the captured graphs hold
the pointers. The decode step is a chain of ~100 small kernel launches per
layer-stack pass; at batch<32 launch overhead is a visible fraction of the
step, so the whole step (embed → layers → lm_head → slot math) is captured
per batch-size bucket with torch.cuda.CUDAGraph (hipGraph on ROCm) and
replayed. A replay runs `bucket` rows: `load()` points rows [B:bucket] at
the scratch sequence, and nothing writes them afterwards. Without graphs
the tensors are fresh per `load()`, and the block table is the narrow one
`kv.block_table` returns: the attention binding sizes its chunk count, and
so its kernel plan, from that width.

Capture constraints honored: the paged-KV pool is preallocated (kv.py), all
shapes are static per bucket, the HIP kernels allocate nothing and never
sync, sampling stays outside the graph (RNG).
"""
from __future__ import annotations

import logging
from typing import Dict, List, Optional, Sequence

import torch

logger = logging.getLogger("bee2bee_amd.engine")


def decode_slot_mapping(
    block_table: torch.Tensor, positions: torch.Tensor, block_size: int
) -> torch.Tensor:
    """slot[b] = block_table[b][pos//bs]*bs + pos%bs, computed on device."""
    blk_idx = torch.div(positions, block_size, rounding_mode="floor")
    blk = block_table.gather(1, blk_idx.unsqueeze(1).long()).squeeze(1)
    return blk * block_size + positions % block_size


class DecodeGraphs:
    """Per-batch-bucket captured decode steps over shared static buffers."""

    def __init__(self, runner, max_batch: int, max_blocks_per_seq: int) -> None:
        self.runner = runner
        self.device = runner.device
        self.max_batch = max_batch
        self.width = max_blocks_per_seq
        dev = self.device
        self.input_ids = torch.zeros(max_batch, dtype=torch.int64, device=dev)
        self.positions = torch.zeros(max_batch, dtype=torch.int32, device=dev)
        self.seq_lens = torch.ones(max_batch, dtype=torch.int32, device=dev)
        self.block_table = torch.zeros(
            max_batch, self.width, dtype=torch.int32, device=dev
        )
        self.logits: Dict[int, torch.Tensor] = {}
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._pool = None

    def buckets(self) -> list:
        out, b = [], 1
        while b < self.max_batch:
            out.append(b)
            b *= 2
        out.append(self.max_batch)
        return out

    def bucket_for(self, batch: int) -> int:
        for b in self.buckets():
            if batch <= b:
                return b
        return self.max_batch

    def _run(self, B: int) -> torch.Tensor:
        ids = self.input_ids[:B]
        pos = self.positions[:B]
        bt = self.block_table[:B]
        lens = self.seq_lens[:B]
        slots = decode_slot_mapping(bt, pos, self.runner.kv.block_size)
        hidden = self.runner.forward_decode(ids, pos, slots, bt, lens)
        return self.runner.lm_head(hidden)

    def _capture(self, B: int) -> None:
        torch.cuda.synchronize()
        # warmup on a side stream (required before capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._run(B)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        if self._pool is None:
            with torch.cuda.graph(g):
                self.logits[B] = self._run(B)
            self._pool = g.pool()
        else:
            with torch.cuda.graph(g, pool=self._pool):
                self.logits[B] = self._run(B)
        self._graphs[B] = g
        logger.info("captured decode graph for batch bucket %d", B)

    def run(self, batch: int) -> torch.Tensor:
        """Replay (capturing on first use) and return logits [bucket, V]
        for the rows DecodeState.load() wrote."""
        B = self.bucket_for(batch)
        if B not in self._graphs:
            self._capture(B)
        # ALWAYS consume a replay, never the capture run itself: library
        # GEMMs may pick a different algorithm while capturing, so replayed
        # steps would not be bit-identical with the capture step otherwise.
        self._graphs[B].replay()
        return self.logits[B]


class DecodeState:
    """The four decode inputs of one sequence list, and the ids sampled for
    it: see the module docstring."""

    def __init__(self, runner, graphs: Optional[DecodeGraphs],
                 scratch_seq: int) -> None:
        self.runner = runner
        self.kv = runner.kv
        self.graphs = graphs
        self.scratch_seq = scratch_seq
        self.seqs: Optional[List[int]] = None  # list the rows were loaded for
        self._pending: Optional[torch.Tensor] = None
        self.ids = self.pos = self.lens = self.bt = None

    def load(self, seq_ids: Sequence[int], last_ids: Sequence[int],
             lengths: Sequence[int]) -> None:
        """Full rebuild from host lists: sequence i feeds last_ids[i] at
        position lengths[i] (its tokens already in the cache)."""
        B, g = len(seq_ids), self.graphs
        pos = torch.tensor(lengths, dtype=torch.int32)
        bt = self.kv.block_table(seq_ids)
        if g is None:
            dev = self.runner.device
            self.ids = torch.empty(B, dtype=torch.int64, device=dev)
            self.pos = torch.empty(B, dtype=torch.int32, device=dev)
            self.lens = torch.empty(B, dtype=torch.int32, device=dev)
            self.bt = bt
        else:
            self.ids, self.pos, self.lens, self.bt = (
                g.input_ids[:B], g.positions[:B], g.seq_lens[:B],
                g.block_table[:B])
            self.bt[:, : bt.shape[1]].copy_(bt, non_blocking=True)
            bucket = g.bucket_for(B)
            if bucket > B:  # pad rows -> scratch sequence, length 1
                sb = self.kv.block_table([self.scratch_seq])[0]
                g.block_table[B:bucket, : sb.shape[0]].copy_(sb)
                g.positions[B:bucket].zero_()
                g.seq_lens[B:bucket].fill_(1)
                g.input_ids[B:bucket].zero_()
        self.ids.copy_(torch.tensor(last_ids, dtype=torch.int64),
                       non_blocking=True)
        self.pos.copy_(pos, non_blocking=True)
        self.lens.copy_(pos + 1, non_blocking=True)
        self.seqs = list(seq_ids)
        self._pending = None

    def advance(self, next_ids: torch.Tensor, refresh_tables: bool) -> None:
        """In-place bump to the next token of the same sequences; device
        ops only. refresh_tables re-reads the block tables: a sequence
        crossed a page boundary or released a window page."""
        self.ids.copy_(next_ids)
        self.pos.add_(1)
        self.lens.add_(1)
        if refresh_tables:
            bt = self.kv.block_table(self.seqs)
            if self.graphs is None:
                self.bt = bt
            else:
                self.bt[:, : bt.shape[1]].copy_(bt, non_blocking=True)
        self._pending = None

    def logits(self) -> torch.Tensor:
        """Run the step over the loaded rows: logits [B, V]."""
        if self.graphs is not None:
            B = len(self.seqs)
            return self.graphs.run(B)[:B]
        slots = decode_slot_mapping(self.bt, self.pos, self.kv.block_size)
        hidden = self.runner.forward_decode(
            self.ids, self.pos, slots, self.bt, self.lens)
        return self.runner.lm_head(hidden)

    def hold(self, seq_ids: Sequence[int], next_ids: torch.Tensor) -> None:
        """Keep next_ids [B], sampled on device for seq_ids, as the next
        step's inputs (no host round trip). Ids of any other list than the
        loaded one are not kept: bumping with them fed a request its
        neighbour's token."""
        self._pending = next_ids if list(seq_ids) == self.seqs else None

    def pending(self, seq_ids: Sequence[int]) -> Optional[torch.Tensor]:
        """The held ids if the rows can be bumped for seq_ids, else None
        (rebuild): the state was loaded for exactly this list and holds
        ids sampled for it."""
        return self._pending if list(seq_ids) == self.seqs else None

    def forget(self) -> None:
        """The sequences moved on without the state: rebuild next time."""
        self.seqs = self._pending = None
