"""GPU execution mode for YouTube random, channel and snowball sampling.

The device counterpart of :func:`crawler_amd.youtube.runner.run_youtube`
for ``sampling_method`` ``random``, ``channel`` and ``snowball``. For the
same index, ``min_channel_videos``, limit, ``max_searches``,
``daily_quota``, ``max_depth``, rng seed, crawl label and ``now`` it
writes byte-identical per-channel ``posts.jsonl`` files, returns the same
stats dict and raises :class:`QuotaExceeded` where the CPU client lets
one escape.

Random sampling runs in ROUNDS of many prefixes (search, first-claim of
the ids, first-claim of the channels: csrc/yt_sample.hip); only four
integers per search come back to the host, where
:func:`replay_random_accounting` replays ``get_random_videos``' quota and
batching bookkeeping to find the search at which the CPU loop stops. A
round draws all its prefixes before that search is known, so the GPU
mode may consume MORE prefixes from the rng than the CPU loop does: the
rng's end state differs, nothing else.

Snowball sampling runs one BFS LAYER at a time (first-claim of the
frontier's channel indices, uploads, then csrc/yt_snowball.hip: a scan of
the layer's generated description bytes for ``UC...`` ids and a lookup of
each hit in a device reverse map of the universe's channel ids). Only the
per-channel upload counts come back to the host, where
:class:`SnowballReplay` replays ``get_snowball_videos``' quota and the
``limit`` cut. The CPU client's per-text dedup and its ``not in visited``
filter on the next frontier are not mirrored: the frontier skips visited
and repeated ids when it is consumed, so neither is observable.

Deliberate differences from the CPU runner, all outside what it can
express: an unknown ``UC...`` url raises ``ValueError`` (the CPU runner
spends a unit and writes nothing in channel mode, and crawls nothing from
that seed in snowball mode); in channel and snowball mode a video-channel
lookup that does not fit the quota raises ``QuotaExceeded`` (the CPU
conversion pool swallows it and emits the post without channel data);
and snowball resolves a discovered id against the whole universe, where
the CPU index knows only the ids it has generated so far (every id a
generated description carries is one of those, so crawls agree; should
two channel indices share an id, the device takes the smaller index and
the CPU index the one registered last).
"""
from __future__ import annotations

import datetime as _dt
import random
import time as _time
from typing import List, Optional, Sequence, Tuple

from .client import (QUOTA_DAILY, QUOTA_LIST, QUOTA_SEARCH, QuotaExceeded,
                     SyntheticYouTubeClient)
from .synth import SyntheticYouTubeIndex

_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)
DEFAULT_MAX_SEARCHES = 200


class RandomReplay:
    """Incremental replay of ``SyntheticYouTubeClient.get_random_videos``'
    bookkeeping over per-search integer rows
    ``(invalid, candidates, new_channels, verified)``."""

    def __init__(self, limit: int, max_searches: int, daily_quota: int):
        self.limit = limit
        self.max_searches = max_searches
        self.daily_quota = daily_quota
        self.quota_used = 0
        self.videos = 0      # len(videos)
        self.queued = 0      # len(queued_ids)
        self.searches = 0
        self.done = False    # the sampling loop has ended
        self._returned = False  # ... by the in-loop return (no flush)
        self._finished = False
        self.stats = {"searches": 0, "video_batches": 0,
                      "channels_checked": 0, "gate_rejected": 0,
                      "invalid_ids": 0}

    def _spend(self, units: int):
        if self.quota_used + units > self.daily_quota:
            raise QuotaExceeded(
                f"daily quota exceeded: {self.quota_used}+{units}")
        self.quota_used += units

    def _list_videos(self, count: int):
        for _ in range(0, count, 50):
            self._spend(QUOTA_LIST)
            self.stats["video_batches"] += 1

    def wants_search(self) -> bool:
        return (not self.done and self.videos + self.queued < self.limit
                and self.searches < self.max_searches)

    def feed(self, rows: Sequence[Sequence[int]]) -> int:
        """Consume rows until the loop ends or they run out; returns how
        many were consumed."""
        used = 0
        for inv, cand, newch, ver in rows:
            if not self.wants_search():
                self.done = True
                break
            if self.quota_used + QUOTA_SEARCH > self.daily_quota:
                self.done = True   # the client's try/except: break
                break
            self.quota_used += QUOTA_SEARCH
            self.stats["searches"] += 1
            self.searches += 1
            used += 1
            self.stats["invalid_ids"] += inv
            if cand:
                self._list_videos(cand)
                for _ in range(newch):
                    self._spend(QUOTA_LIST)
                self.stats["channels_checked"] += cand
                self.stats["gate_rejected"] += cand - ver
            self.queued += ver
            while self.queued >= 50 or (
                    self.queued and self.videos + self.queued >= self.limit):
                b = min(50, self.queued)
                self.queued -= b
                self._list_videos(b)
                self.videos += b
                if self.videos >= self.limit:
                    self.done = self._returned = True
                    return used
        if not self.wants_search():
            self.done = True
        return used

    def finish(self) -> int:
        """The final flush; returns the number of accepted videos."""
        if not self._finished:
            self._finished = True
            self.done = True
            if not self._returned and self.queued:
                self._list_videos(self.queued)
                self.videos += self.queued
                self.queued = 0
        return max(0, min(self.videos, self.limit))


def replay_random_accounting(rows, limit: int, max_searches: int,
                             daily_quota: int
                             ) -> Tuple[int, int, dict, int]:
    """Replay ``get_random_videos(limit, max_searches)`` on integers.

    ``rows[s] = (invalid, candidates, new_channels, verified)`` for the
    s-th search: ids failing the validity rule, rule-valid ids not seen
    before, distinct channels among those not looked up before, and
    candidates passing the ``video_count > min_channel_videos`` gate.
    Returns ``(n_accepted, cut_search, stats, quota_used)``: the accepted
    videos are the first ``n_accepted`` verified ids of searches
    ``< cut_search``. Raises QuotaExceeded where the client would. Rows
    running out ends sampling like the ``max_searches`` bound does."""
    rp = RandomReplay(limit, max_searches, daily_quota)
    cut = rp.feed(rows)
    n = rp.finish()
    return n, cut, dict(rp.stats), rp.quota_used


class SnowballReplay:
    """Integer replay of ``SyntheticYouTubeClient.get_snowball_videos``
    over the upload counts of the channels it visits, in visiting order.

    A channel with no uploads costs nothing; any other costs its
    Videos.List units for the WHOLE channel before the ``limit`` cut is
    looked at. ``videos`` is the number of videos to take so far (the
    first ``videos`` uploads in channel order) and ``done`` is set once
    the limit is reached: the client returns there."""

    def __init__(self, limit: int, daily_quota: int):
        self.limit = limit
        self.daily_quota = daily_quota
        self.quota_used = 0
        self.videos = 0
        self.done = limit <= 0
        self.stats = {"searches": 0, "video_batches": 0,
                      "channels_checked": 0, "gate_rejected": 0,
                      "invalid_ids": 0}

    _spend = RandomReplay._spend
    _list_videos = RandomReplay._list_videos

    def feed(self, counts: Sequence[int]) -> int:
        """Consume per-channel upload counts until the limit cuts or they
        run out; returns how many channels were consumed. Raises
        QuotaExceeded where ``list_videos`` would."""
        used = 0
        for c in counts:
            if self.done:
                break
            used += 1
            if c <= 0:
                continue
            self._list_videos(c)
            self.videos += min(c, self.limit - self.videos)
            if self.videos >= self.limit:
                self.done = True
        return used


# ---------- device side ----------

def _floor_secs(t: _dt.datetime) -> Tuple[int, bool]:
    if t.tzinfo is None:
        t = t.replace(tzinfo=_dt.timezone.utc)
    d = t - _EPOCH
    secs = d // _dt.timedelta(seconds=1)
    return secs, (d - _dt.timedelta(seconds=secs)) > _dt.timedelta(0)


def _fanout_channels() -> int:
    """Channels handed to the file sink in one call. The sink keeps up to
    256 files open between calls and opens one more per channel during a
    call, so a call gets at most half of the process's open-file limit
    less those 256, and never more than 8192."""
    try:
        import resource

        soft = resource.getrlimit(resource.RLIMIT_NOFILE)[0]
    except (ImportError, OSError, ValueError):
        return 128
    if soft == resource.RLIM_INFINITY:
        return 8192
    return max(64, min(8192, soft // 2 - 256))


def _resolve_channel_urls(index: SyntheticYouTubeIndex,
                          urls: List[str]) -> List[int]:
    ns = []
    for s in urls:
        if s.startswith("UC"):
            n = index.channel_index_of(s)
            if n is None:
                raise ValueError(f"unknown YouTube channel id: {s}")
        else:
            n = int(s)
        ns.append(n)
    return ns


def _sample_random(index, limit, min_channel_videos, rng, max_searches,
                   daily_quota, round_searches, dev, claim_slots_log2,
                   timings):
    import numpy as np
    import torch

    from ..ops import gpu

    rp = RandomReplay(limit, max_searches, daily_quota)
    seen = gpu.YtFirstClaim(dev, slots_log2=claim_slots_log2)
    chans = gpu.YtFirstClaim(dev, slots_log2=claim_slots_log2)
    accepted = []
    s0 = 0
    slots = gpu.YT_SEARCH_SLOTS
    while rp.wants_search():
        S = min(round_searches, max_searches - s0)
        pref = np.frombuffer(
            "".join(SyntheticYouTubeClient.generate_random_prefix(rng)
                    for _ in range(S)).encode("ascii"),
            dtype=np.uint8).reshape(S, 5)
        r = gpu.yt_search(index, torch.from_numpy(pref.copy()).to(dev))
        flags = r["flags"].reshape(-1)
        present = (flags & 1) != 0
        valid = (flags & 2) != 0
        first = seen.claim(r["keys"], valid, s0 * slots).bool()
        new_ch = chans.claim(r["chan"], first, s0 * slots).bool()
        verified = first & (r["vcount"] > min_channel_videos)
        rows = torch.stack([
            (present & ~valid).view(S, slots).sum(1),
            first.view(S, slots).sum(1),
            new_ch.view(S, slots).sum(1),
            verified.view(S, slots).sum(1),
        ], dim=1).cpu().tolist()
        accepted.append(r["ids"].view(-1, 11)[verified])
        rp.feed(rows)
        s0 += S
    n = rp.finish()
    timings["claim_grown"] = seen.grown + chans.grown
    if accepted:
        ids = torch.cat(accepted)[:n]
    else:
        ids = torch.empty((0, 11), dtype=torch.uint8, device=dev)
    return ids, rp


def _sample_channels(index, urls, limit, daily_quota, dev):
    import torch

    from ..ops import gpu

    ns = _resolve_channel_urls(index, urls)
    rp = RandomReplay(0, 0, daily_quota)   # quota + stats holder
    looked_up = set()
    if not ns:
        return (torch.empty((0, 11), dtype=torch.uint8, device=dev), rp,
                looked_up)
    chans = torch.tensor(ns, dtype=torch.int64, device=dev)
    ids, counts = gpu.yt_uploads(index, chans, limit)
    for n, c in zip(ns, counts.cpu().tolist()):
        if n not in looked_up:
            rp._spend(QUOTA_LIST)          # get_channel_info
            looked_up.add(n)
        rp._list_videos(c)                 # get_channel_videos
    k = torch.arange(gpu.YT_UPLOAD_SLOTS, device=dev)
    take = k[None, :] < counts[:, None]
    return ids[take], rp, looked_up


def _sample_snowball(index, urls, limit, max_depth, daily_quota, dev,
                     claim_slots_log2, chunk_videos, timings):
    import torch

    from ..ops import gpu
    from .batch import yt_descriptions_from_ids_device

    ns = _resolve_channel_urls(index, urls)
    if any(n < 0 for n in ns):
        raise ValueError("a YouTube channel index cannot be negative")
    rp = SnowballReplay(limit, daily_quota)
    visited = gpu.YtFirstClaim(dev, slots_log2=claim_slots_log2)
    rmap = None
    accepted = []
    frontier = torch.tensor(ns, dtype=torch.int64, device=dev)
    k = torch.arange(gpu.YT_UPLOAD_SLOTS, device=dev)
    base_idx = 0
    depth = 0
    # ``timings["snowball_steps"] = {}`` asks for the layer loop's own
    # split; it costs a device synchronisation per step
    steps = timings.get("snowball_steps")
    t0 = _time.perf_counter()

    def lap(name):
        nonlocal t0
        if steps is not None:
            torch.cuda.synchronize(dev)
            now_ = _time.perf_counter()
            steps[name] = steps.get(name, 0.0) + now_ - t0
            t0 = now_

    while frontier.numel() and not rp.done and depth <= max_depth:
        # `visited`: the frontier's first occurrences, in global order
        first = visited.claim(frontier, None, base_idx).bool()
        base_idx += int(frontier.numel())
        chans = frontier[first]
        lap("claim")
        ids, counts = gpu.yt_uploads(index, chans, gpu.YT_UPLOAD_SLOTS)
        before = rp.videos
        rp.feed(counts.cpu().tolist())
        layer = ids[k[None, :] < counts[:, None]][:rp.videos - before]
        accepted.append(layer)
        lap("uploads_replay")
        depth += 1
        if rp.done or depth > max_depth:
            break
        # discovery: scan the layer's description bytes, resolve the hits
        if rmap is None:
            rmap = gpu.YtChannelReverseMap(index, dev)
            lap("reverse_map_build")
        nxt = []
        for c0 in range(0, int(layer.shape[0]), chunk_videos):
            pool, d_off, d_len = yt_descriptions_from_ids_device(
                index, layer[c0:c0 + chunk_videos])
            lap("describe")
            hit_off, _ = gpu.yt_scan_channel_ids(pool, d_off, d_len)
            lap("scan")
            n = rmap.lookup(pool, hit_off)
            nxt.append(n[n >= 0])
            lap("lookup")
        frontier = (torch.cat(nxt) if nxt else
                    torch.empty(0, dtype=torch.int64, device=dev))
    timings["claim_grown"] = visited.grown
    timings["snowball_layers"] = depth
    if accepted:
        ids = torch.cat(accepted)
    else:
        ids = torch.empty((0, 11), dtype=torch.uint8, device=dev)
    return ids, rp


def run_youtube_gpu(cfg, urls: List[str], *, sm=None, rng=None, now=None,
                    max_searches: Optional[int] = None,
                    daily_quota: Optional[int] = None,
                    round_searches: int = 4096, device="cuda:0",
                    claim_slots_log2: int = 16, index=None,
                    chunk_videos: int = 1 << 18,
                    timings: Optional[dict] = None) -> dict:
    """Random / channel / snowball YouTube sampling on the GPU; see the
    module doc.

    ``round_searches`` prefixes are searched per round; ``chunk_videos``
    (<= 1M: the batch offsets are int32) bounds one generate+encode
    batch and one snowball description scan. ``timings``, when given,
    receives the wall-clock split."""
    import torch

    from ..config import calculate_date_filters
    from ..engine.state import LocalStateManager
    from ..ops import gpu
    from .batch import build_batch_from_ids_device, yt_meta_from_ids_device

    method = cfg.sampling_method
    if method not in ("random", "channel", "snowball"):
        raise ValueError(
            f"the YouTube GPU mode covers random, channel and snowball "
            f"sampling, not {method!r}")
    if not 1 <= chunk_videos <= 1_000_000:
        raise ValueError("chunk_videos must be in 1..1000000")
    seed = getattr(cfg, "synthetic_seed", 99)
    index = index or SyntheticYouTubeIndex(seed=seed)
    rng = rng or random.Random(seed)
    if max_searches is None:
        max_searches = getattr(cfg, "yt_max_searches", DEFAULT_MAX_SEARCHES)
    if daily_quota is None:
        daily_quota = getattr(cfg, "yt_daily_quota", QUOTA_DAILY)
    sm = sm or LocalStateManager(cfg)
    limit = cfg.max_posts if cfg.max_posts > 0 else 100
    dev = torch.device(device)
    t = timings if timings is not None else {}
    for k in ("sample", "gen_encode", "d2h", "fanout"):
        t.setdefault(k, 0.0)
    tick = _time.perf_counter

    t0 = tick()
    with torch.cuda.device(dev):
        if method == "random":
            ids, rp = _sample_random(
                index, limit, cfg.min_channel_videos, rng, max_searches,
                daily_quota, max(1, round_searches), dev,
                claim_slots_log2, t)
            looked_up = None
        elif method == "snowball":
            ids, rp = _sample_snowball(
                index, urls, limit, max(cfg.max_depth, 1), daily_quota,
                dev, claim_slots_log2, chunk_videos, t)
            looked_up = set()   # sampling never calls get_channel_info
        else:
            ids, rp, looked_up = _sample_channels(index, urls, limit,
                                                  daily_quota, dev)

        # date window as a device mask on `published`
        meta = yt_meta_from_ids_device(index, ids)
        n_chan = meta["n_chan"]
        from_t, to_t = calculate_date_filters(cfg)
        if from_t is not None:
            lo, frac = _floor_secs(from_t)
            lo += 1 if frac else 0
            hi, _ = _floor_secs(to_t)
            keep = (meta["published"] >= lo) & (meta["published"] <= hi)
            ids, n_chan = ids[keep], n_chan[keep]
        n_videos = int(ids.shape[0])

        if looked_up is not None and n_videos:
            # the conversion pool's get_channel_info(v.channel_id):
            # random sampling has every video's channel cached already
            for n in torch.unique(n_chan).cpu().tolist():
                if n not in looked_up:
                    rp._spend(QUOTA_LIST)

        # stable sort by channel: each channel's lines contiguous, in
        # their sampled order
        order = torch.sort(n_chan, stable=True).indices
        ids = ids[order].contiguous()
        torch.cuda.synchronize(dev)
        t["sample"] += tick() - t0

        posts = 0
        fanout_channels = _fanout_channels()
        ar24 = torch.arange(24, device=dev)
        for c0 in range(0, n_videos, chunk_videos):
            t0 = tick()
            b = build_batch_from_ids_device(
                index, ids[c0:c0 + chunk_videos], dev, cfg.crawl_label)
            out, line_off, line_len = gpu.yt_parse_encode(b, now=now)
            # rows are channel-sorted, so the first-appearance channel
            # table is sorted too and channel c owns one run of rows
            cnt = torch.bincount(b.channel_idx.to(torch.int64),
                                 minlength=b.n_channels)
            end = torch.cumsum(cnt, 0)
            lo_b = line_off[end - cnt]
            hi_b = line_off[end - 1] + line_len[end - 1].to(torch.int64)
            cids = b.pool[b.ch_id_off.to(torch.int64)[:, None] + ar24]
            torch.cuda.synchronize(dev)
            t["gen_encode"] += tick() - t0

            t0 = tick()
            buf = out.cpu().numpy()
            lo_h, hi_h = lo_b.cpu().tolist(), hi_b.cpu().tolist()
            cid_blob = cids.cpu().numpy().tobytes().decode("ascii")
            t["d2h"] += tick() - t0
            t["jsonl_bytes"] = t.get("jsonl_bytes", 0) + int(buf.shape[0])

            t0 = tick()
            items = [(cid_blob[24 * c:24 * c + 24], lo_h[c], hi_h[c])
                     for c in range(b.n_channels)]
            # the sink closes surplus files only between calls, so one
            # call must not open more files than the process may hold
            mv = memoryview(buf)
            for i0 in range(0, len(items), fanout_channels):
                sm.store_post_lines_batch(items[i0:i0 + fanout_channels],
                                          mv)
            posts += b.n
            t["fanout"] += tick() - t0

    t0 = tick()
    sm.save_state()
    sm.close()
    t["fanout"] += tick() - t0
    return {
        "videos": n_videos,
        "posts": posts,
        "quota_used": rp.quota_used,
        **rp.stats,
    }
