"""What the BFS engine (engine/gpu_runner.py) and the random walk
(engine/gpu_randomwalk.py) share: the fetch stage in front of parse+encode,
the per-channel byte ranges of the encoded lines and the pinned spill ring.

Fetch rule: with a fetch window (ops.gpu.window_params: --date-between,
--max-posts, --sample-size, or forced) a chunk goes through the
fetch-window kernel (csrc/fetch_window.hip, the row form of
fetch_channel_messages' walk) and only the kept rows, gathered by the
compact-rows kernel, are encoded, claimed and written: a channel then owns
kept[k] lines, not P, and one with no kept row writes and truncates
nothing. Without sampling the kept set is the CPU path's. With
--sample-size the two paths agree in the sample's size, in drawing a
uniform subset of the same window and in being deterministic, but not in
WHICH posts are drawn or in their order: the CPU path shuffles with
Python's random (Fisher-Yates) and writes the sample in shuffled order;
this path keeps the sample_size smallest splitmix64 keys of (--sample-seed,
chat_id, msg_id) and writes them in row order, so the sample does not
depend on how channels are chunked. Without a window no new kernel is
launched. --max-comments clamps the rows' comment counts
(ops.gpu.cap_comments) before parse+encode, windowed or not.

Deadend rule: with --time-ago (ops.gpu.gate_params) the window is forced
and the channel gate (csrc/channel_gate.hip, the row form of
is_channel_active) follows it: a channel whose newest fetched message, or
whose newest message at all when nothing was fetched, is not newer than
the cutoff is inactive. It loses its rows, so it writes and truncates
nothing and none of its links is claimed; what else a deadend means is the
engine's business. With --sample-size the newest FETCHED message is the
newest of each path's own sample, so the CPU and the GPU crawl can
disagree on a deadend exactly where their samples differ.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch


def cid_of(username: str, universe: int) -> Optional[int]:
    """The universe id of a synthetic channel name, or None."""
    if username.startswith("c") and username[1:].isdigit():
        cid = int(username[1:])
        if cid < universe:
            return cid
    return None


def padded_name_rows(names: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """Zero the bytes of uint8[n, w] name rows past lens[n] ON THE GPU, so
    a D2H ships clean fixed-width byte strings."""
    col = torch.arange(names.shape[1], device=names.device, dtype=lens.dtype)
    return torch.where(col[None, :] < lens[:, None], names,
                       torch.zeros_like(names))


def comment_cap(cfg) -> Optional[int]:
    """--max-comments, or None without a cap (unset or negative)."""
    cap = getattr(cfg, "max_comments", None)
    return None if cap is None or cap < 0 else int(cap)


class FetchStage:
    """The plan (window, gate, max_comments; None = not asked for) that a
    CrawlerConfig resolves to, and its application to a K x P batch."""

    def __init__(self, gpu, cfg, force_window: bool):
        self.gpu = gpu
        self.gate = gpu.gate_params(cfg)
        # the gate needs keep/kept, so it forces the window kernel too
        self.window = gpu.window_params(
            cfg, force=force_window or self.gate is not None)
        self.max_comments = comment_cap(cfg)

    def apply(self, batch):
        """``(batch to encode, kept_k, active_k, row_channel)``. Without a
        window only the comment cap applies and the other three are None.
        With one, the batch holds the kept rows only (None when the chunk
        keeps no row), ``kept_k`` is int64[K] rows per channel,
        ``active_k`` bool[K] (None without a gate) and ``row_channel`` the
        device int32 row-to-channel map of the kept rows."""
        gpu = self.gpu
        if self.window is None:
            return gpu.cap_comments(batch, self.max_comments), None, None, None
        keep, kept = gpu.fetch_window(batch, **self.window)
        active_k = None
        if self.gate is not None:
            keep, kept, active, _latest = gpu.channel_gate(
                batch, keep, kept, **self.gate)
            active_k = active.cpu().numpy() != 0
        kept_k = kept.cpu().numpy().astype(np.int64)
        if not kept_k.any():
            return None, kept_k, active_k, None
        from ..ops import batch as _B
        rows, row_channel = gpu.compact_rows(batch, keep, kept)
        batch = gpu.cap_comments(_B.select_rows(batch, rows),
                                 self.max_comments)
        return batch, kept_k, active_k, row_channel


def channel_ranges(line_off, line_len, K: int, P: int, kept_k=None):
    """``(lo_k, hi_k, n_lines_k)``: the byte range [lo, hi) that each of K
    channels owns in the encoded buffer and how many of its lines were
    written (``line_len > 0``). Lines are grouped by channel: P each, or
    kept_k[k] each for a windowed batch. Vectorized: a python loop over
    numpy scalars costs ~0.3s per 1500 channels."""
    if kept_k is None:
        off2 = line_off.reshape(K, P)
        len2 = line_len.reshape(K, P)
        return off2[:, 0], off2[:, -1] + len2[:, -1], (len2 > 0).sum(axis=1)
    # windowed: channel k owns the kept[k] lines from the exclusive cumsum
    # of kept on; none = an empty range
    end_k = np.cumsum(kept_k)
    beg_k = end_k - kept_k
    written = np.concatenate(([0], np.cumsum(line_len > 0, dtype=np.int64)))
    n_lines_k = written[end_k] - written[beg_k]
    if not len(line_off):
        zero = np.zeros(K, dtype=np.int64)
        return zero, zero, n_lines_k
    some = kept_k > 0
    last = np.maximum(end_k - 1, 0)
    lo_k = np.where(some, line_off[np.minimum(beg_k, last)], 0)
    hi_k = np.where(some, line_off[last] + line_len[last], 0)
    return lo_k, hi_k, n_lines_k


class SpillRing:
    """Two reusable pinned host slots for the encoded JSONL, one sink
    ticket per slot. A slot's previous ticket is awaited before a D2H may
    overwrite it, which makes the spill pipeline two batches deep: batch
    i's disk writes run under the GPU work of batches i+1 and i+2. (A
    pinned allocation per batch cost ~0.1s: the d2h phase was
    allocation-bound, not copy-bound.)"""

    def __init__(self, sm):
        self.sm = sm
        self._slots = [None, None]
        self._tickets = [None, None]
        self._next = 0

    def claim(self) -> int:
        """Take the next slot and retire its old ticket. MAIN THREAD ONLY:
        the native sink's ticket wait also evicts surplus fds and must not
        race a concurrent submit."""
        slot = self._next
        self._next = 1 - slot
        self.wait(slot)
        return slot

    def stage(self, slot: int, out_dev: torch.Tensor) -> torch.Tensor:
        """Issue the non-blocking D2H of ``out_dev`` into the slot (grown
        with 1/8 headroom when too small); the caller synchronises before
        it reads the returned pinned view."""
        need = int(out_dev.numel())
        if self._slots[slot] is None or self._slots[slot].numel() < need:
            self._slots[slot] = torch.empty(
                need + need // 8, dtype=torch.uint8, pin_memory=True)
        out_host = self._slots[slot][:need]
        out_host.copy_(out_dev, non_blocking=True)
        return out_host

    def submit(self, slot: int, items, buf) -> None:
        """One fan-out call: the native sink appends all ``(name, lo, hi)``
        of ``buf`` in parallel with the GIL released."""
        self._tickets[slot] = self.sm.store_post_lines_batch(
            items, buf, ticket=True)

    def wait(self, slot: int) -> None:
        self.sm.wait_post_write(self._tickets[slot])
        self._tickets[slot] = None

    def drain(self) -> None:
        """Wait out all in-flight ticketed sink writes."""
        for slot in (0, 1):
            self.wait(slot)
        self.sm.drain_post_writes()
