"""ctypes driver for the CDNA4 hot-path kernels (ops/csrc/libcrawlhip.so).

The HIP extension is built in-tree by ``__graft_entry__.build()`` (or
``python -m crawler_amd.ops.build``) with hipcc --offload-arch=gfx950.
On a GPU host the extension is REQUIRED: :func:`require_lib` raises rather
than letting callers silently fall back to the (1000x slower) Python path.
"""
from __future__ import annotations

import ctypes
import dataclasses
import datetime as _dt
import os
from typing import List, Optional, Tuple

import torch

from ..models.post import format_go_time
from . import batch as B
from . import views

_CSRC = os.path.dirname(os.path.abspath(__file__)) + "/csrc"
_LIB_PATH = os.path.join(_CSRC, "libcrawlhip.so")

MAX_LINKS = 8

_lib = None

# Every extern "C" entry point of csrc/*.hip -> its argument types, in the
# C definition's order; all return int (tests/test_gpu_bindings.py pins
# the names and counts to the sources). The last argument of every
# launching entry point is the stream.
_vp_t, _ll, _cl, _ci = (ctypes.c_void_p, ctypes.c_longlong, ctypes.c_long,
                        ctypes.c_int)
_pp = ctypes.POINTER(ctypes.c_void_p)   # void**: a pointer array
_lp = ctypes.POINTER(ctypes.c_long)     # const long*: a scalar array
_SIGNATURES = {
    # parse_encode.hip
    "crawl_batch_ptr_count": [],
    "crawl_stage_budget": [],
    "crawl_measure_extract": [_pp, _lp, _pp, _vp_t, _ci, _vp_t],
    "crawl_write": [_pp, _lp, _pp, _vp_t, _vp_t, _vp_t, _ci, _vp_t],
    "crawl_write_lds": [_pp, _lp, _pp, _vp_t, _vp_t, _vp_t, _ci, _vp_t],
    "crawl_write_staged": [_pp, _lp, _pp, _vp_t, _vp_t, _vp_t, _ci, _ci,
                           _ci, _ci, _ci, _vp_t],
    "crawl_write_scratch": [_pp, _lp, _pp, _vp_t, _cl, _vp_t, _vp_t, _ci,
                            _vp_t],
    "crawl_compact": [_vp_t, _cl, _vp_t, _vp_t, _vp_t, _ci, _ci, _vp_t],
    # dedup.hip
    "crawl_claim_links": [_vp_t, _vp_t, _ci, _ci, _vp_t, _ll, _vp_t, _vp_t,
                          _ci, _vp_t],
    "crawl_bloom_update": [_vp_t, _vp_t, _ci, _ci, _vp_t, _ll, _ci, _vp_t],
    "crawl_claim_compact": [_vp_t, _vp_t, _vp_t, _vp_t, _ci, _ci, _vp_t,
                            _vp_t, _vp_t, ctypes.c_uint, _ci, _vp_t],
    "crawl_insert_hashes": [_vp_t, _cl, _vp_t, _ll, _ci, _vp_t],
    # feedgen.hip
    "crawl_feed_meta": [_pp, _lp, _vp_t, _pp, _ci, _vp_t],
    "crawl_feed_fill": [_pp, _lp] + [_vp_t] * 5 + [_pp, _ci, _vp_t],
    "crawl_feed_comments": [_pp, _lp, _vp_t, _vp_t, _cl, _vp_t, _cl, _cl,
                            _pp, _ci, _vp_t],
    # aggregate.hip, sample.hip, htmlclass.hip
    "crawl_channel_stats": [_vp_t] * 4 + [_ci, _ci] + [_vp_t] * 5 + [_vp_t],
    "crawl_reservoir_sample": [_cl, _ci, _ci, _ci, _vp_t, _ci, _vp_t],
    "crawl_html_classify": [_vp_t, _vp_t, _vp_t, _ci, _vp_t, _vp_t, _ci,
                            _vp_t],
    # fetch_window.hip
    "crawl_fetch_window": [_vp_t, _vp_t, _vp_t, _ci, _ci] + [_cl] * 5
                          + [_vp_t, _vp_t, _ci, _vp_t],
    # channel_gate.hip
    "crawl_channel_gate": [_vp_t, _vp_t, _ci, _ci, _cl] + [_vp_t] * 4
                          + [_ci, _vp_t],
    "crawl_compact_rows": [_vp_t, _vp_t, _ci, _ci, _vp_t, _vp_t, _ci,
                           _vp_t],
    # yt_encode.hip
    "crawl_yt_ptr_count": [],
    "crawl_yt_measure": [_pp, _lp, _vp_t, _ci, _vp_t],
    "crawl_yt_write": [_pp, _lp, _vp_t, _vp_t, _ci, _vp_t],
    # yt_feedgen.hip
    "crawl_yt_gen_ids": [_ll, _ll, _ll, _vp_t, _vp_t],
    "crawl_yt_gen_meta": [_ll] * 4 + [_vp_t] * 11 + [_vp_t],
    "crawl_yt_gen_fill": [_ll] * 3 + [_vp_t] * 6 + [_vp_t],
    "crawl_yt_chan_lens": [_ll, _vp_t, _ll, _vp_t, _vp_t, _vp_t, _vp_t],
    "crawl_yt_gen_channels": [_ll, _ll, _vp_t, _ll] + [_vp_t] * 9 + [_vp_t],
    # yt_sample.hip
    "crawl_yt_search": [_ll, _ll, _vp_t, _ll] + [_vp_t] * 5 + [_vp_t],
    "crawl_yt_claim_insert": [_vp_t, _vp_t, _vp_t, _ll, _ll, _vp_t, _vp_t,
                              _ci, _vp_t, _vp_t],
    "crawl_yt_first_claim": [_vp_t, _vp_t, _ll, _ll, _vp_t, _vp_t, _ci,
                             _vp_t, _vp_t, _vp_t],
    "crawl_yt_uploads": [_ll, _vp_t, _ll, _ci, _vp_t, _vp_t, _vp_t],
    # yt_snowball.hip
    "crawl_yt_scan_count": [_vp_t, _vp_t, _vp_t, _ll, _vp_t, _vp_t],
    "crawl_yt_scan_write": [_vp_t, _vp_t, _vp_t, _ll, _vp_t, _vp_t, _vp_t],
    "crawl_yt_cid_table_build": [_ll, _ll, _vp_t, _ci, _vp_t, _vp_t],
    "crawl_yt_cid_lookup": [_ll, _vp_t, _vp_t, _ll, _vp_t, _ci, _vp_t,
                            _vp_t],
}


def lib_available() -> bool:
    return os.path.exists(_LIB_PATH)


def load_lib():
    global _lib
    if _lib is not None:
        return _lib
    lib = ctypes.CDLL(_LIB_PATH)
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = argtypes
    _lib = lib
    return lib


def require_lib():
    """On a GPU host, a missing/failed extension is an ERROR, not a fallback."""
    if _lib is None and not lib_available():
        raise RuntimeError(
            "libcrawlhip.so not built — run __graft_entry__.build() "
            "(hipcc --offload-arch=gfx950) before GPU execution; the Python "
            "golden path is not a substitute on GPU hosts"
        )
    return load_lib()


def _cur_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _call(name: str, *args, stream: Optional[torch.cuda.Stream] = None):
    """Run the launching entry point ``name``: tensor arguments (or None)
    pass as their device pointers, and the stream argument that ends every
    such signature is ``stream``, by default the current one. A non-zero
    return raises."""
    args = [_vp(a) if a is None or isinstance(a, torch.Tensor) else a
            for a in args]
    args.append(_cur_stream() if stream is None
                else ctypes.c_void_p(stream.cuda_stream))
    rc = getattr(require_lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed: hip {rc}")


def _excl_offsets(lengths: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """Measure-then-place: (int64 exclusive offsets, host total) of integer
    ``lengths``, with one host sync (none for empty input)."""
    end = torch.cumsum(lengths, 0, dtype=torch.int64)
    return end - lengths, int(end[-1].item()) if lengths.numel() else 0


def _kp_shape(batch: B.MessageBatch) -> Tuple[int, int]:
    """(K, P) of a K x P channel-grouped batch."""
    K = batch.n_channels
    P = batch.n // K if K else 0
    assert K * P == batch.n, "batch must be K x P channel-grouped"
    return K, P


class YtEncodeResult(tuple):
    """``(out, line_off, line_len)`` of yt_parse_encode. ``raw`` is the
    guarded allocation ``out`` is a view into (test seam ``_guard`` > 0),
    else None."""

    raw: Optional[torch.Tensor] = None

    def __new__(cls, out, line_off, line_len, raw=None):
        self = super().__new__(cls, (out, line_off, line_len))
        self.raw = raw
        return self


def yt_parse_encode(batch, now: Optional[_dt.datetime] = None,
                    grid: int = 0, *, _poison: Optional[int] = None,
                    _guard: int = 0) -> Tuple[torch.Tensor, torch.Tensor,
                                              torch.Tensor]:
    """YouTube batch -> (out bytes, line_off, line_len); byte-identical to
    youtube.batch.encode_yt_batch.

    ``_poison`` / ``_guard`` are the test seams of :func:`parse_encode`
    (off by default): the guarded buffer is the result's ``.raw``."""
    lib = require_lib()
    dev = batch.device
    assert dev.type == "cuda"
    n = batch.n
    if n == 0:
        # nothing to launch: (0 + 3) // 4 blocks is an invalid grid
        out, raw = _alloc_out(0, dev, _poison, _guard)
        return YtEncodeResult(
            out, torch.zeros(0, dtype=torch.int64, device=dev),
            torch.zeros(0, dtype=torch.int32, device=dev), raw)
    now = now or _dt.datetime.now(_dt.timezone.utc)
    created = format_go_time(now.replace(microsecond=0)).encode()
    capture = format_go_time(now).encode()
    to_dev = lambda b: torch.frombuffer(bytearray(b or b"\0"),
                                        dtype=torch.uint8).to(dev)
    from ..youtube.batch import LANGS

    extras = {"label": to_dev(batch.crawl_label.encode()),
              "lang_pool": to_dev("".join(LANGS).encode()),
              "created_str": to_dev(created), "capture_str": to_dev(capture)}
    ptrs = views.bind("YtView", views.lookup_in(batch, extras), dev)
    assert len(ptrs) == lib.crawl_yt_ptr_count(), "library older than views.h"
    scalars = (ctypes.c_long * 4)(
        n, len(batch.crawl_label.encode()), len(created), len(capture)
    )
    if grid <= 0:
        grid = min((n + 3) // 4, 8192)
    line_len = torch.zeros(n, dtype=torch.int32, device=dev)
    _call("crawl_yt_measure", ptrs, scalars, line_len, grid)
    line_off, total = _excl_offsets(line_len)
    out, raw = _alloc_out(total, dev, _poison, _guard)
    _call("crawl_yt_write", ptrs, scalars, line_off, out, grid)
    return YtEncodeResult(out, line_off, line_len, raw)


# ---------- YouTube sampling (csrc/yt_sample.hip) ----------

YT_SEARCH_SLOTS = 17   # n_valid <= 5, n_noise <= 12
YT_UPLOAD_SLOTS = 29   # video_count <= 29


def yt_search(index, prefixes: torch.Tensor) -> dict:
    """SyntheticYouTubeIndex.search_prefix + the client's validity rule
    for ``prefixes`` (uint8[S,5] on the device). Returns per-slot
    tensors over S*17 slots: ``ids`` uint8[S,17,11], ``flags`` uint8[S,17]
    (bit 0 present, bit 1 rule-valid), and for rule-valid slots ``keys``
    (exact 64-bit id key), ``chan`` (channel index) and ``vcount`` (that
    channel's video_count)."""
    dev = prefixes.device
    assert dev.type == "cuda" and prefixes.dtype == torch.uint8
    prefixes = prefixes.reshape(-1, 5).contiguous()
    S = prefixes.shape[0]
    m = S * YT_SEARCH_SLOTS
    out = {
        "ids": torch.empty((S, YT_SEARCH_SLOTS, 11), dtype=torch.uint8,
                           device=dev),
        "flags": torch.empty((S, YT_SEARCH_SLOTS), dtype=torch.uint8,
                             device=dev),
        "keys": torch.empty(m, dtype=torch.int64, device=dev),
        "chan": torch.empty(m, dtype=torch.int64, device=dev),
        "vcount": torch.empty(m, dtype=torch.int32, device=dev),
    }
    _call("crawl_yt_search", index.seed, index.universe, prefixes, S,
          out["ids"], out["flags"], out["keys"], out["chan"], out["vcount"])
    return out


def yt_uploads(index, chans: torch.Tensor, limit: int):
    """SyntheticYouTubeIndex.channel_uploads for channel indices
    ``chans`` (int64[K] on the device): (ids uint8[K,29,11], counts
    int32[K]); slot k of row c is an upload iff k < counts[c]."""
    dev = chans.device
    assert dev.type == "cuda" and chans.dtype == torch.int64
    chans = chans.contiguous()
    K = chans.numel()
    ids = torch.empty((K, YT_UPLOAD_SLOTS, 11), dtype=torch.uint8,
                      device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    limit = max(0, min(int(limit), YT_UPLOAD_SLOTS))
    _call("crawl_yt_uploads", index.seed, chans, K, limit, ids, counts)
    return ids, counts


class YtClaimTableError(RuntimeError):
    """The first-claim table's device error word was set: a probe wrapped
    the whole table (full), or a key equalled the empty sentinel."""


class YtFirstClaim:
    """Deterministic first-occurrence marking over 64-bit keys.

    An open-addressing table in HBM (keys + min global index). ``claim``
    returns, for each masked-in element, whether it is the first
    occurrence of its key over every claim so far; elements are numbered
    by the caller's global index (``base_idx + i``), so the answer does
    not depend on thread scheduling. The table grows by doubling to keep
    the load <= 0.5 (``grow=False`` pins its size: a full table raises
    :class:`YtClaimTableError`)."""

    _EMPTY = -1  # all-ones; real keys are < 2**63

    def __init__(self, device, slots_log2: int = 16, grow: bool = True):
        self.device = torch.device(device)
        self.grow = grow
        self.grown = 0
        require_lib()
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._alloc(slots_log2)
        self._bound = 0  # upper bound on the distinct keys held

    def _alloc(self, slots_log2: int):
        self.slots_log2 = slots_log2
        cap = 1 << slots_log2
        self.keys = torch.full((cap,), self._EMPTY, dtype=torch.int64,
                               device=self.device)
        self.min_idx = torch.full((cap,), -1, dtype=torch.int64,
                                  device=self.device)

    def _check(self):
        e = int(self._err.item())
        if e:
            self._err.zero_()
            raise YtClaimTableError(
                f"first-claim table error word {e:#x} "
                f"(slots=2**{self.slots_log2})")

    def _reserve(self, incoming: int):
        if not self.grow:
            return
        cap = 1 << self.slots_log2
        if 2 * (self._bound + incoming) <= cap:
            return
        # recount exactly, then double until the load fits; re-insert
        # the retained (key, first index) pairs with the pass-1 kernel
        live = self.keys != self._EMPTY
        old_k = self.keys[live].contiguous()
        old_i = self.min_idx[live].contiguous()
        self._bound = int(old_k.numel())
        log2 = self.slots_log2
        while 2 * (self._bound + incoming) > (1 << log2):
            log2 += 1
            self.grown += 1
        if log2 == self.slots_log2:
            return
        self._alloc(log2)
        _call("crawl_yt_claim_insert", old_k, None, old_i, old_k.numel(), 0,
              self.keys, self.min_idx, self.slots_log2, self._err)
        self._check()

    def claim(self, keys: torch.Tensor, mask: Optional[torch.Tensor],
              base_idx: int) -> torch.Tensor:
        """keys int64[n]; mask uint8[n]/bool[n] or None (all in).
        Returns uint8[n]: 1 = first occurrence."""
        assert keys.dtype == torch.int64 and keys.device == self.device
        keys = keys.contiguous()
        n = keys.numel()
        first = torch.zeros(n, dtype=torch.uint8, device=self.device)
        if n == 0:
            return first
        if mask is not None:
            mask = mask.to(torch.uint8).contiguous()
            assert mask.numel() == n
            incoming = int(mask.count_nonzero().item())
        else:
            incoming = n
        self._reserve(incoming)
        _call("crawl_yt_first_claim", keys, mask, n, int(base_idx),
              self.keys, self.min_idx, self.slots_log2, first, self._err)
        self._bound += incoming
        self._check()
        return first


# ---------- YouTube snowball discovery (csrc/yt_snowball.hip) ----------

YT_CID_LEN = 24   # 'UC' + 22 characters


def yt_scan_channel_ids(pool: torch.Tensor, text_off: torch.Tensor,
                        text_len: torch.Tensor):
    """Leftmost non-overlapping matches of ``UC[0-9A-Za-z_-]{22}`` in the
    texts ``pool[text_off[t] : text_off[t] + text_len[t]]`` (uint8 pool,
    int64[n] offsets, int32[n] lengths, all on the device): the bytes
    regex's ``finditer`` starts. Returns ``(hit_off int64[m], counts
    int32[n])``: every match's absolute pool offset, in text order then
    match order, and the per-text match count. A match lies wholly inside
    its text; texts may be packed back to back."""
    dev = pool.device
    assert dev.type == "cuda" and pool.dtype == torch.uint8
    assert text_off.dtype == torch.int64 and text_len.dtype == torch.int32
    assert text_off.device == dev and text_len.device == dev
    pool = pool.contiguous()
    text_off = text_off.contiguous()
    text_len = text_len.contiguous()
    n = text_off.numel()
    assert text_len.numel() == n
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), counts
    len64 = text_len.to(torch.int64)
    bad = ((text_off < 0) | (len64 < 0)
           | (text_off + len64 > pool.numel())).any()
    if bool(bad.item()):
        raise ValueError("a text range lies outside the pool")
    _call("crawl_yt_scan_count", pool, text_off, text_len, n, counts)
    out_base, total = _excl_offsets(counts)
    hit_off = torch.empty(total, dtype=torch.int64, device=dev)
    if total:
        _call("crawl_yt_scan_write", pool, text_off, text_len, n, out_base,
              hit_off)
    return hit_off, counts


class YtChannelReverseMap:
    """Channel id -> channel index for a whole synthetic universe: the
    device counterpart of ``SyntheticYouTubeIndex.channel_index_of`` with
    every channel registered.

    An open-addressing table of channel indices in HBM, built once per
    ``(seed, universe)`` and sized for a load <= 0.5 (``slots_log2`` pins
    the size instead: a full table raises :class:`YtClaimTableError`).
    No strings are stored; a lookup regenerates the slot's id and
    compares all 24 bytes. An id two indices share maps to the smaller."""

    def __init__(self, index, device, slots_log2: Optional[int] = None):
        self.device = torch.device(device)
        assert self.device.type == "cuda"
        self.seed = int(index.seed)
        self.universe = int(index.universe)
        if self.universe <= 0:
            raise ValueError("the universe must hold at least one channel")
        if slots_log2 is None:
            slots_log2 = 1
            while (1 << slots_log2) < 2 * self.universe:
                slots_log2 += 1
        self.slots_log2 = int(slots_log2)
        with torch.cuda.device(self.device):
            self.table = torch.full((1 << self.slots_log2,), -1,
                                    dtype=torch.int64, device=self.device)
            err = torch.zeros(1, dtype=torch.int32, device=self.device)
            _call("crawl_yt_cid_table_build", self.seed, self.universe,
                  self.table, self.slots_log2, err)
            e = int(err.item())
        if e:
            raise YtClaimTableError(
                f"channel reverse map error word {e:#x} "
                f"(slots=2**{self.slots_log2}, universe={self.universe})")

    def lookup(self, pool: torch.Tensor,
               hit_off: torch.Tensor) -> torch.Tensor:
        """Channel index of the 24 bytes at each ``pool`` offset (int64[m]
        on the device), or -1 where they name no channel."""
        assert pool.dtype == torch.uint8 and pool.device == self.device
        assert hit_off.dtype == torch.int64 and hit_off.device == self.device
        pool = pool.contiguous()
        hit_off = hit_off.contiguous()
        m = hit_off.numel()
        out = torch.empty(m, dtype=torch.int64, device=self.device)
        if m == 0:
            return out
        bad = ((hit_off < 0) | (hit_off + YT_CID_LEN > pool.numel())).any()
        if bool(bad.item()):
            raise ValueError("an id offset lies outside the pool")
        _call("crawl_yt_cid_lookup", self.seed, pool, hit_off, m, self.table,
              self.slots_log2, out)
        return out


def channel_stats(batch: B.MessageBatch, line_len=None):
    """Segmented per-channel engagement aggregation (SURVEY §2.6:
    GetTotalChannelViews etc. -> one workgroup per channel segment).
    Returns dict of device tensors: views/forwards/replies int64[K],
    posts int32[K], totals int64[4] (views,forwards,replies,posts).

    ``line_len`` (int32[n] on the batch's device, e.g. an EncodeResult's)
    restricts ``posts`` to the rows with ``line_len > 0``. The kernel adds
    into ``totals``, so the driver hands it zeros. A batch without
    channels gives empty outputs and no launch."""
    dev = batch.device
    K, P = _kp_shape(batch)
    if line_len is not None:
        if (line_len.dtype != torch.int32 or line_len.numel() != batch.n
                or line_len.device != dev):
            raise ValueError(
                f"line_len must be int32[{batch.n}] on {dev}, got "
                f"{line_len.dtype}[{line_len.numel()}] on {line_len.device}")
        line_len = line_len.contiguous()
    out = {
        "views": torch.zeros(K, dtype=torch.int64, device=dev),
        "forwards": torch.zeros(K, dtype=torch.int64, device=dev),
        "replies": torch.zeros(K, dtype=torch.int64, device=dev),
        "posts": torch.zeros(K, dtype=torch.int32, device=dev),
        "totals": torch.zeros(4, dtype=torch.int64, device=dev),
    }
    if K == 0:
        return out
    m = batch.meta
    _call("crawl_channel_stats", m["views"], m["forwards"], m["reply_count"],
          line_len, P, K, out["views"], out["forwards"], out["replies"],
          out["posts"], out["totals"])
    return out


def reservoir_sample(batch: B.MessageBatch, k: int, seed: int = 0):
    """Per-channel uniform sample without replacement (SURVEY §2.6
    Fisher-Yates row). Returns int32[K, min(k, P)] global row indices
    (device): a channel with no more than ``k`` rows keeps all of them,
    as the reference does (telegramutils.go:124)."""
    dev = batch.device
    K, P = _kp_shape(batch)
    if k < 0:
        raise ValueError("the sample size must not be negative")
    k = min(k, P)
    out = torch.zeros((K, k), dtype=torch.int32, device=dev)
    if K == 0 or k == 0:
        return out
    _call("crawl_reservoir_sample", seed, P, K, k, out,
          min(max(1, (K + 3) // 4), 8192))
    return out


def reservoir_sample_oracle(P: int, K: int, k: int, seed: int = 0):
    """Python replay of the device reservoir (same splitmix stream);
    like the driver, it keeps min(k, P) rows per channel."""
    k = min(k, P)

    def sm64(x):
        z = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        return z ^ (z >> 31)

    out = []
    for c in range(K):
        slot = list(range(c * P, c * P + k))
        for i in range(k, P):
            r = sm64((seed ^ ((c * 0x9E3779B1 + i) & (2**64 - 1)))
                     & (2**64 - 1))
            j = r % (i + 1)
            if j < k:
                slot[j] = c * P + i
        out.append(slot)
    return out


class FetchWindowResult(tuple):
    """``(keep, kept)`` of fetch_window. ``raw_keep`` / ``raw_kept`` are
    the guarded allocations they are views into (test seam ``_guard`` >
    0), else None."""

    raw_keep: Optional[torch.Tensor] = None
    raw_kept: Optional[torch.Tensor] = None

    def __new__(cls, keep, kept, raw_keep=None, raw_kept=None):
        self = super().__new__(cls, (keep, kept))
        self.raw_keep = raw_keep
        self.raw_kept = raw_kept
        return self


def fetch_window(batch: B.MessageBatch, stop_below: Optional[int] = None,
                 skip_above: Optional[int] = None, cap: int = 0,
                 sample_k: int = 0, seed: int = 0, *,
                 _poison: Optional[int] = None, _guard: int = 0):
    """Which rows of a K x P channel-grouped batch the crawl keeps
    (FetchChannelMessagesWithSampling, telegramutils.go:25-157; oracle:
    golden_window.fetch_window). Per channel, newest row first: a row
    dated after ``skip_above`` is skipped, the first other row dated
    before ``stop_below`` ends the walk, and so does the ``cap``-th
    candidate (0 = no cap); of more than ``sample_k`` candidates (0 = no
    sampling) the ``sample_k`` with the smallest
    ``golden_window.sample_key`` stay. Bounds are unix seconds, None =
    unbounded; ``seed`` is taken modulo 2**64.

    Returns ``(keep uint8[n], kept int32[K])`` on the batch's device.
    The kernel writes every element of both. A batch without channels
    gives empty outputs and no launch.

    ``_poison`` / ``_guard`` are the test seams of :func:`parse_encode`
    (off by default): the guarded buffers are the result's ``.raw_keep``
    and ``.raw_kept`` (``_guard`` counts elements)."""
    dev = batch.device
    K, P = _kp_shape(batch)
    if cap < 0 or sample_k < 0:
        raise ValueError("cap and sample_k must not be negative")
    keep, raw_keep = _alloc_out(batch.n, dev, _poison, _guard)
    kept, raw_kept = _alloc_out(K, dev, _poison, _guard, torch.int32)
    if K == 0:
        return FetchWindowResult(keep, kept, raw_keep, raw_kept)
    from .golden_window import NO_SKIP, NO_STOP

    clamp = lambda v: max(NO_STOP, min(NO_SKIP, int(v)))
    lo = NO_STOP if stop_below is None else clamp(stop_below)
    hi = NO_SKIP if skip_above is None else clamp(skip_above)
    seed = ((int(seed) + (1 << 63)) % (1 << 64)) - (1 << 63)
    date = batch.meta["date"]
    for nm, t, dt_ in (("date", date, torch.int32),
                       ("chat_id", batch.chat_id, torch.int64),
                       ("msg_id", batch.msg_id, torch.int64)):
        assert t.dtype == dt_ and t.device == dev and t.is_contiguous(), nm
        assert t.numel() == batch.n, nm
    _call("crawl_fetch_window", date, batch.chat_id, batch.msg_id, P, K, lo,
          hi, int(cap), int(sample_k), seed, keep, kept,
          min((K + 3) // 4, 8192))
    return FetchWindowResult(keep, kept, raw_keep, raw_kept)


def window_params(cfg, force: bool = False) -> Optional[dict]:
    """The :func:`fetch_window` arguments a CrawlerConfig asks for, or
    None when the GPU crawl's per-row ``min_post_date`` filter already
    does all of it (no date-between window, no ``max_posts`` cap, no
    sampling). ``force=True`` never returns None: a caller that needs
    ``keep`` and ``kept`` anyway (the channel gate, the random walk) gets
    the walk that ``min_post_date`` alone stops, or one without bounds,
    which is exactly the CPU walk's fetched set. Precedence is
    ``engine.pipeline.fetch_channel_messages``':
    both date-between bounds set -> that window, ``min_post_date``
    ignored; otherwise ``min_post_date`` alone stops the walk. Sampling
    needs ``date_between_min`` (``_maybe_sample``). The CPU compares
    integer dates with float timestamps: ``d > hi`` is ``d > floor(hi)``
    and ``d < lo`` is ``d < ceil(lo)``."""
    import math

    stop = skip = None
    window = (cfg.date_between_min is not None
              and cfg.date_between_max is not None)
    if window:
        stop = math.ceil(cfg.date_between_min.timestamp())
        skip = math.floor(cfg.date_between_max.timestamp())
    elif cfg.min_post_date is not None:
        stop = math.ceil(cfg.min_post_date.timestamp())
    cap = cfg.max_posts if cfg.max_posts and cfg.max_posts > 0 else 0
    sample_k = (cfg.sample_size
                if (cfg.sample_size and cfg.sample_size > 0
                    and cfg.date_between_min is not None) else 0)
    if not force and not window and cap == 0 and sample_k == 0:
        return None
    return {"stop_below": stop, "skip_above": skip, "cap": int(cap),
            "sample_k": int(sample_k),
            "seed": int(getattr(cfg, "sample_seed", 0))}


def gate_params(cfg) -> Optional[dict]:
    """The :func:`channel_gate` cutoff a CrawlerConfig asks for
    (``--time-ago``), or None without one. ``is_channel_active`` compares
    integer dates with a float timestamp: ``d > ts`` is ``d > floor(ts)``."""
    import math

    if cfg.post_recency is None:
        return None
    return {"recency": math.floor(cfg.post_recency.timestamp())}


def _grouped_shape(batch: B.MessageBatch, keep, kept):
    """(K, P) of a K x P channel-grouped batch, after checking a
    fetch-window result against it."""
    dev = batch.device
    K, P = _kp_shape(batch)
    for nm, t, dt_, n in (("keep", keep, torch.uint8, batch.n),
                          ("kept", kept, torch.int32, K)):
        assert t.dtype == dt_ and t.device == dev and t.is_contiguous(), nm
        assert t.numel() == n, nm
    return K, P


def channel_gate(batch: B.MessageBatch, keep: torch.Tensor,
                 kept: torch.Tensor, recency: int, *,
                 _poison: Optional[int] = None):
    """The activity deadend (``is_channel_active``) over a batch that
    went through :func:`fetch_window` (csrc/channel_gate.hip; oracle:
    golden_gate.channel_gate). A channel's newest date is the greatest
    date of its kept rows, or, with none kept, the date of its row with
    the greatest ``msg_id``; the channel is active iff that date is later
    than ``recency`` (unix seconds; a tie is inactive). An inactive
    channel loses its kept rows: ``keep`` and ``kept`` are updated IN
    PLACE.

    Returns ``(keep, kept, active uint8[K], latest int32[K])``. The kernel
    writes every element of ``active`` and ``latest``; ``_poison`` (test
    seam) fills both with that byte first. A batch without rows gives
    all-inactive outputs and no launch."""
    dev = batch.device
    K, P = _grouped_shape(batch, keep, kept)
    active, _ = _alloc_out(K, dev, _poison, 0)
    latest, _ = _alloc_out(K, dev, _poison, 0, torch.int32)
    if K == 0 or P == 0:
        active.zero_()
        latest.zero_()
        return keep, kept, active, latest
    from .golden_window import NO_SKIP, NO_STOP

    recency = max(NO_STOP, min(NO_SKIP, int(recency)))
    date = batch.meta["date"]
    for nm, t, dt_ in (("date", date, torch.int32),
                       ("msg_id", batch.msg_id, torch.int64)):
        assert t.dtype == dt_ and t.device == dev and t.is_contiguous(), nm
        assert t.numel() == batch.n, nm
    _call("crawl_channel_gate", date, batch.msg_id, P, K, recency, keep,
          kept, active, latest, min((K + 3) // 4, 8192))
    return keep, kept, active, latest


def compact_rows(batch: B.MessageBatch, keep: torch.Tensor,
                 kept: torch.Tensor, *, _poison: Optional[int] = None):
    """The kept rows of a windowed batch as indices
    (csrc/channel_gate.hip; oracle: golden_gate.compact_rows): ``(rows
    int64[sum(kept)], row_channel int32[sum(kept)])``, the global row
    indices channel by channel and ascending within one, which is
    ``keep.nonzero()``, and the channel each row belongs to. ``kept`` must
    count the non-zero ``keep`` bytes per channel, as :func:`fetch_window`
    and :func:`channel_gate` leave it; a channel's surplus rows would be
    dropped, never written past its range. Nothing kept gives empty
    outputs and no launch."""
    dev = batch.device
    K, P = _grouped_shape(batch, keep, kept)
    kept_offset = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    if K:
        if bool((kept < 0).any().item()):
            raise ValueError("kept must not be negative")
        torch.cumsum(kept, 0, dtype=torch.int64, out=kept_offset[1:])
    total = int(kept_offset[-1].item())
    rows, _ = _alloc_out(total, dev, _poison, 0, torch.int64)
    row_channel, _ = _alloc_out(total, dev, _poison, 0, torch.int32)
    if total == 0:
        return rows, row_channel
    _call("crawl_compact_rows", keep, kept_offset, P, K, rows, row_channel,
          min((K + 3) // 4, 8192))
    return rows, row_channel


def cap_comments(batch: B.MessageBatch, max_comments: int):
    """``--max-comments`` over a batch: a thread keeps its first
    ``max_comments`` comments (``get_message_comments``), none with 0; a
    negative value means no cap and returns the batch itself. Only the
    rows' ``com_cnt`` column is replaced (clamped copy); the comment
    table is shared and untouched, and parse+encode takes a thread's
    length from ``com_cnt`` alone."""
    if max_comments is None or max_comments < 0:
        return batch
    meta = dict(batch.meta)
    meta["com_cnt"] = meta["com_cnt"].clamp(max=int(max_comments))
    return dataclasses.replace(batch, meta=meta)


_HTML_STATUS = ["valid", "not_channel", "invalid"]
_HTML_REASON = ["", "not_supergroup", "not_found", "not_found",
                "unrecognized"]


def html_classify(docs, device="cuda:0"):
    """Batch t.me HTML classification on GPU (oracle:
    engine.htmlvalidator.parse_channel_html). docs: list[bytes].
    Returns list of (status, reason) strings."""
    dev = torch.device(device)
    n = len(docs)
    blob = b"".join(docs) or b"\0"
    pool = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    offs, cur = [], 0
    lens = []
    for d in docs:
        offs.append(cur)
        lens.append(len(d))
        cur += len(d)
    doc_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    doc_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    reason = torch.zeros(n, dtype=torch.int32, device=dev)
    _call("crawl_html_classify", pool, doc_off, doc_len, n, status, reason,
          min(max(1, (n + 3) // 4), 8192))
    st = status.cpu().numpy()
    rs = reason.cpu().numpy()
    return [(_HTML_STATUS[int(st[i])], _HTML_REASON[int(rs[i])])
            for i in range(n)]


# Emoji / content-type constant tables shipped to the device once.
def _const_tables(device):
    epool = b"".join(e.encode("utf-8") for e in B.EMOJI_TABLE)
    eoff, cur = [], 0
    elen = []
    for e in B.EMOJI_TABLE:
        n = len(e.encode("utf-8"))
        eoff.append(cur)
        elen.append(n)
        cur += n
    cpool = b"".join(c.encode() for c in B.CONTENT_TYPES)
    coff, ccur = [], 0
    clen = []
    for c in B.CONTENT_TYPES:
        coff.append(ccur)
        clen.append(len(c))
        ccur += len(c)
    t = lambda x, dt_: torch.tensor(x, dtype=dt_, device=device)
    return {
        "emoji_pool": torch.frombuffer(bytearray(epool), dtype=torch.uint8).to(device),
        "emoji_off": t(eoff, torch.int32),
        "emoji_len": t(elen, torch.int32),
        "ctname_pool": torch.frombuffer(bytearray(cpool), dtype=torch.uint8).to(device),
        "ctname_off": t(coff, torch.int32),
        "ctname_len": t(clen, torch.int32),
    }


_tables_cache = {}


def const_tables(device):
    key = str(device)
    if key not in _tables_cache:
        _tables_cache[key] = _const_tables(device)
    return _tables_cache[key]


@dataclasses.dataclass
class EncodeResult:
    """Device-side results of one parse+encode pass."""

    out: torch.Tensor        # uint8[total_bytes] JSONL (concatenated lines)
    line_off: torch.Tensor   # int64[N] start offset of each line
    line_len: torch.Tensor   # int32[N] (0 = filtered by min_post_date)
    link_name: torch.Tensor  # uint8[N, MAX_LINKS, 32]
    link_len: torch.Tensor   # uint8[N, MAX_LINKS]
    link_src: torch.Tensor   # uint8[N, MAX_LINKS]
    link_cnt: torch.Tensor   # int32[N]
    link_hash: torch.Tensor  # int64[N, MAX_LINKS] (fnv1a64 bits)
    writer: str = ""         # staged | plain | lds | scratch ("" = no launch)
    # test seam: the guarded allocation ``out`` is a view into (_guard > 0)
    raw: Optional[torch.Tensor] = None


def _stride_bound(batch: B.MessageBatch) -> int:
    """Sound per-message upper bound on the JSONL line length.

    Worst-case expansion of any escaped byte is 6x; the constant skeleton,
    numeric fields and timestamps fit in the 2200-byte base. Comment text /
    handle / reaction contributions are segment-summed per message."""
    m = batch.meta
    dev = batch.device
    i64 = lambda t: t.to(torch.int64)
    c = m["channel_idx"].to(torch.int64)
    bound = (
        2200
        + 6 * i64(m["text_len"]) + 6 * i64(m["aux_len"])
        + 12 * i64(batch.ch_title_len[c])
        + 36 * i64(batch.ch_user_len[c])
        + 6 * i64(m["poster_len"])
        + 45 * i64(m["react_cnt"])
        + 170 * i64(m["com_cnt"])
        + 35 * MAX_LINKS
    )
    ccnt = i64(m["com_cnt"])
    total_c = int(ccnt.sum().item())
    if total_c:
        # segment sums through a prefix array indexed by com_off/com_cnt:
        # a row subset (select_rows) shares the full comment table, so
        # the table is not simply the rows' segments laid end to end
        extra = (6 * (i64(batch.com_text_len) + i64(batch.com_handle_len))
                 + 45 * i64(batch.com_react_cnt))
        pre = torch.zeros(extra.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(extra, 0, out=pre[1:])
        c0 = i64(m["com_off"])
        bound = bound + pre[c0 + ccnt] - pre[c0]
    return int(bound.max().item())


# per-line staged extras beyond the text fields: outlink names
# (8 x 32 + 8) + reaction id/count ints (2 x 64 x 4) + alignment slack
_STAGE_FIXED = 812
# staged kernel's block-table caps (parse_encode.hip TG_*_CAP)
_EMOJI_POOL_CAP, _EMOJI_CAP, _TS_CAP = 512, 64, 64
_CTNAME_POOL_CAP, _CTNAME_CAP = 512, 32


def _tables_fit(tables, created, capture) -> bool:
    """True when the per-batch tables fit the staged writer's block caps."""
    return not (tables["emoji_pool"].numel() > _EMOJI_POOL_CAP
                or tables["emoji_off"].numel() > _EMOJI_CAP
                or tables["ctname_pool"].numel() > _CTNAME_POOL_CAP
                or tables["ctname_off"].numel() > _CTNAME_CAP
                or len(created) > _TS_CAP or len(capture) > _TS_CAP)


def _stage_need(batch) -> int:
    """Worst-case per-line bytes the staged writer carves from its
    per-wave LDS stage for this batch (user+title+poster+desc +
    links/reactions); cached per batch."""
    need = getattr(batch, "_stage_need", None)
    if need is None:
        m = batch.meta
        need = _STAGE_FIXED
        if batch.n:
            need += (max(int(m["text_len"].max().item()),
                         int(m["aux_len"].max().item()))
                     + int(m["poster_len"].max().item()))
        if batch.n_channels:
            need += (int(batch.ch_user_len.max().item())
                     + int(batch.ch_title_len.max().item()))
        try:
            batch._stage_need = need
        except AttributeError:
            pass
    return need


_stage_budget_cache = None


def _stage_budget(lib) -> int:
    global _stage_budget_cache
    if _stage_budget_cache is None:
        _stage_budget_cache = int(lib.crawl_stage_budget())
    return _stage_budget_cache


def _stage_fits(batch, lib, tables, created, capture) -> bool:
    """True when every line's staged fields (user+title+poster+desc +
    links/reactions) fit the staged writer's per-wave LDS budget AND
    the per-batch tables fit its block caps."""
    if os.environ.get("CRAWL_NO_STAGED") == "1":
        return False
    if not _tables_fit(tables, created, capture):
        return False
    return _stage_need(batch) <= _stage_budget(lib)


def _pick_writer(env, single_pass: bool, stage_need: Optional[int],
                 budget: int) -> str:
    """Which JSONL writer parse_encode runs: "scratch" (single-pass
    scratch + compaction), "lds" (CRAWL_LDS_WRITE set), "staged" (the
    batch's staged bytes fit the LDS budget) or "plain".

    ``env`` is the environment mapping; ``stage_need`` is
    :func:`_stage_need` of the batch, or None when the per-batch tables
    exceed the staged writer's block caps; ``budget`` is
    crawl_stage_budget()."""
    if single_pass:
        return "scratch"
    if env.get("CRAWL_LDS_WRITE"):
        return "lds"
    if env.get("CRAWL_NO_STAGED") == "1":
        return "plain"
    if stage_need is not None and stage_need <= budget:
        return "staged"
    return "plain"


def _alloc_out(total: int, dev, poison: Optional[int], guard: int,
               dtype=torch.uint8):
    """Output allocation: (out, raw) of ``total`` elements. With the test
    seams off this is a bare torch.empty and raw is None. ``guard`` > 0
    places ``out`` inside a larger buffer with ``guard`` poisoned elements
    on each side (raw is that buffer); ``poison`` fills every byte of
    ``out`` too, so a writer that skips one cannot inherit a stale correct
    value from the allocator."""
    if poison is None and guard <= 0:
        return torch.empty(total, dtype=dtype, device=dev), None
    guard = max(guard, 0)
    raw = torch.empty(total + 2 * guard, dtype=dtype, device=dev)
    if poison is not None:
        raw.view(torch.uint8).fill_(poison)
    else:
        raw[:guard].view(torch.uint8).fill_(0xA5)
        raw[guard + total:].view(torch.uint8).fill_(0xA5)
    return raw[guard:guard + total], raw


def parse_encode(
    batch: B.MessageBatch,
    now: Optional[_dt.datetime] = None,
    min_post_date: Optional[_dt.datetime] = None,
    grid: int = 0,
    stream: Optional[torch.cuda.Stream] = None,
    single_pass: bool = False,
    *,
    _poison: Optional[int] = None,
    _guard: int = 0,
) -> EncodeResult:
    """Parse + JSONL-encode a batch on the current CUDA device.

    Default path: measure+extract then write at exact offsets, with the
    D2H overlap handled by the caller. The single_pass variant (scratch +
    compaction) measured slower on 1.25M-post batches (strided scratch
    thrashes L2) and is kept for experimentation.
    Returns device tensors; the caller D2H-copies ``out`` for the host
    writer. Byte-for-byte equal to golden_batch.encode_batch(...).

    ``_poison`` / ``_guard`` are test seams (off by default): fill the
    output (and single-pass scratch) with a byte before the write, and
    surround ``out`` with that many poisoned bytes (``result.raw``).
    """
    lib = require_lib()
    dev = batch.device
    assert dev.type == "cuda", "parse_encode requires a CUDA (ROCm) batch"
    n = batch.n
    if n == 0:
        # nothing to launch: (0 + 3) // 4 blocks is an invalid grid
        out, raw = _alloc_out(0, dev, _poison, _guard)
        return EncodeResult(
            out=out,
            line_off=torch.zeros(0, dtype=torch.int64, device=dev),
            line_len=torch.zeros(0, dtype=torch.int32, device=dev),
            link_name=torch.empty((0, MAX_LINKS, 32), dtype=torch.uint8,
                                  device=dev),
            link_len=torch.zeros((0, MAX_LINKS), dtype=torch.uint8,
                                 device=dev),
            link_src=torch.zeros((0, MAX_LINKS), dtype=torch.uint8,
                                 device=dev),
            link_cnt=torch.zeros(0, dtype=torch.int32, device=dev),
            link_hash=torch.zeros((0, MAX_LINKS), dtype=torch.int64,
                                  device=dev),
            raw=raw,
        )
    tables = const_tables(dev)

    now = now or _dt.datetime.now(_dt.timezone.utc)
    created = format_go_time(now.replace(microsecond=0)).encode()
    capture = format_go_time(now).encode()
    created_t = torch.frombuffer(bytearray(created), dtype=torch.uint8).to(dev)
    capture_t = torch.frombuffer(bytearray(capture), dtype=torch.uint8).to(dev)

    extras = dict(tables, pool=batch.text_pool, created_str=created_t,
                  capture_str=capture_t)
    batch_ptrs = views.bind("BatchView", views.lookup_in(batch, extras), dev)
    assert len(batch_ptrs) == lib.crawl_batch_ptr_count(), \
        "library older than views.h"

    if min_post_date is not None:
        mpd = int(min_post_date.timestamp())
    else:
        mpd = -(1 << 62)
    scalars = (ctypes.c_long * 5)(n, 1, mpd, len(created), len(capture))

    link_name = torch.empty((n, MAX_LINKS, 32), dtype=torch.uint8, device=dev)
    link_len = torch.zeros((n, MAX_LINKS), dtype=torch.uint8, device=dev)
    link_src = torch.zeros((n, MAX_LINKS), dtype=torch.uint8, device=dev)
    link_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    link_hash = torch.zeros((n, MAX_LINKS), dtype=torch.int64, device=dev)
    line_len = torch.zeros(n, dtype=torch.int32, device=dev)
    link_ptrs = views.bind("LinkOut", {
        "name": link_name, "name_len": link_len, "src": link_src,
        "cnt": link_cnt, "hash": link_hash}.get, dev)

    if grid <= 0:
        grid = min((n + 3) // 4, 8192)

    stage_need = None
    if (not single_pass and not os.environ.get("CRAWL_LDS_WRITE")
            and os.environ.get("CRAWL_NO_STAGED") != "1"
            and _tables_fit(tables, created, capture)):
        stage_need = _stage_need(batch)
    writer = _pick_writer(os.environ, single_pass, stage_need,
                          _stage_budget(lib))

    if writer == "scratch":
        stride = (_stride_bound(batch) + 31) & ~15
        scratch = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        if _poison is not None:
            scratch.fill_(_poison)
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        _call("crawl_write_scratch", batch_ptrs, scalars, link_ptrs, scratch,
              stride, line_len, overflow, grid, stream=stream)
        line_off, total = _excl_offsets(line_len)
        ovf = int(overflow.item())
        if ovf:
            raise RuntimeError(
                f"line overflowed scratch stride ({ovf} > {stride}); "
                "stride bound is unsound for this batch"
            )
        out, raw = _alloc_out(total, dev, _poison, _guard)
        _call("crawl_compact", scratch, stride, line_off, line_len, out, n,
              grid, stream=stream)
    else:
        _call("crawl_measure_extract", batch_ptrs, scalars, link_ptrs,
              line_len, grid, stream=stream)
        line_off, total = _excl_offsets(line_len)
        out, raw = _alloc_out(total, dev, _poison, _guard)
        if writer == "staged":
            # staged writer: escape-scanned fields + reactions +
            # outlinks + per-batch tables go through LDS so in-line
            # loads never wait the store FIFO (profiles/
            # r02_valu_diet.md); host verified everything fits
            _call("crawl_write_staged", batch_ptrs, scalars, link_ptrs,
                  line_off, line_len, out, tables["emoji_off"].numel(),
                  tables["emoji_pool"].numel(), tables["ctname_off"].numel(),
                  tables["ctname_pool"].numel(), grid, stream=stream)
        else:
            _call("crawl_write_lds" if writer == "lds" else "crawl_write",
                  batch_ptrs, scalars, link_ptrs, line_off, line_len, out,
                  grid, stream=stream)

    return EncodeResult(
        out=out, line_off=line_off, line_len=line_len,
        link_name=link_name, link_len=link_len, link_src=link_src,
        link_cnt=link_cnt, link_hash=link_hash, writer=writer, raw=raw,
    )


class SeenSet:
    """Device-resident seen-channel set (hash table + bloom).

    Replaces the reference's DiscoveredChannels map / URL dedup cache
    (state/datamodels.go:118-162, daprstate.go:550-657) with an HBM
    open-addressing table claimed via atomicCAS (exactly-once discovery)
    plus a bitwise-OR-mergeable bloom for cross-rank union over RCCL.
    """

    def __init__(self, device, slots_log2: int = 22, bloom_bits_log2: int = 26):
        self.device = device
        self.slots = 1 << slots_log2
        self.bloom_bits = 1 << bloom_bits_log2
        self.table = torch.zeros(self.slots, dtype=torch.int64, device=device)
        self.bloom = torch.zeros(
            self.bloom_bits // 32, dtype=torch.int32, device=device
        )
        self._n_new = torch.zeros(1, dtype=torch.int32, device=device)
        self.lib = require_lib()

    def claim(self, res: EncodeResult) -> torch.Tensor:
        """Claim every extracted link; returns new_mask uint8[N, MAX_LINKS].

        Also updates the bloom. Reads self.new_count() for the number of
        first-time discoveries in this batch.
        """
        n = res.link_cnt.shape[0]
        new_mask = torch.zeros(
            (n, MAX_LINKS), dtype=torch.uint8, device=self.device
        )
        self._n_new.zero_()
        grid = min((n * MAX_LINKS + 255) // 256, 4096)
        _call("crawl_claim_links", res.link_hash, res.link_cnt, n, MAX_LINKS,
              self.table, self.slots, new_mask, self._n_new, grid)
        _call("crawl_bloom_update", res.link_hash, res.link_cnt, n, MAX_LINKS,
              self.bloom, self.bloom_bits, grid)
        return new_mask

    def new_count(self) -> int:
        return int(self._n_new.item())

    def compact_claimed(self, res: EncodeResult, new_mask: torch.Tensor):
        """Densify the claim winners ON DEVICE: returns
        (names uint8[M, 32] zero-padded, hashes int64[M]) — row order is
        the atomic claim order (consumers sort host-side). Replaces a
        host nonzero+gather+pad over N*MAX_LINKS candidate slots."""
        n = res.link_cnt.shape[0]
        cap = n * MAX_LINKS
        out_names = torch.empty((cap, 32), dtype=torch.uint8,
                                device=self.device)
        out_hashes = torch.empty(cap, dtype=torch.int64,
                                 device=self.device)
        cursor = torch.zeros(1, dtype=torch.int32, device=self.device)
        grid = min((cap + 255) // 256, 4096)
        _call("crawl_claim_compact", new_mask, res.link_name, res.link_len,
              res.link_hash, n, MAX_LINKS, out_names, out_hashes, cursor, cap,
              grid)
        m = int(cursor.item())  # syncs the stream
        return out_names[:m], out_hashes[:m]

    def merge_remote(self, res_or_hashes, dist, world: int,
                     group=None) -> int:
        """Cross-rank seen-set union: exchange this
        rank's newly-claimed hashes with every peer (count-sized
        all-gather over RCCL — NO cap, round 1's silent 64k truncation
        is gone) and insert the remote ones into the local table. Also
        OR-unions the bloom pre-filter. Returns the number of remote
        hashes inserted."""
        from ..parallel import collectives as C

        local = (res_or_hashes if isinstance(res_or_hashes, torch.Tensor)
                 else res_or_hashes.link_hash.flatten())
        per_rank = C.allgather_hashes(local, dist, world,
                                      device=self.device, group=group)
        rank = C._safe_rank(dist, group)
        inserted = 0
        for r, h in enumerate(per_rank):
            if r == rank:
                continue
            h = h[h != 0].to(self.device)
            self.insert_hashes(h)
            inserted += int(h.numel())
        C.bloom_union(self.bloom, dist, world, group=group)
        return inserted

    def insert_hashes(self, hashes: torch.Tensor) -> None:
        """Bulk-insert merged remote hashes (post all-gather)."""
        n = hashes.numel()
        if n == 0:
            return
        grid = min((n + 255) // 256, 4096)
        _call("crawl_insert_hashes", hashes, n, self.table, self.slots, grid)


def fnv1a64(data: bytes) -> int:
    """Python oracle for the device hash (csrc/common.h fnv1a64)."""
    h = 1469598103934665603
    for b in data:
        h ^= b
        h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def links_to_python(res: EncodeResult) -> List[List[Tuple[str, str]]]:
    """Decode the device link output to [(name, source_type), ...] per msg."""
    srcs = ["mention", "text_url", "url", "plaintext"]
    name = res.link_name.cpu().numpy()
    ln = res.link_len.cpu().numpy()
    src = res.link_src.cpu().numpy()
    cnt = res.link_cnt.cpu().numpy()
    out = []
    for i in range(len(cnt)):
        row = []
        for k in range(int(cnt[i])):
            row.append(
                (bytes(name[i, k, : ln[i, k]]).decode(), srcs[int(src[i, k])])
            )
        out.append(row)
    return out
