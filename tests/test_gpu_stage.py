"""The pieces both Telegram GPU engines share (engine/gpu_stage.py), on
the CPU: channel_ranges against a per-channel loop, the SpillRing ticket
protocol against a recording sink, the FetchStage plan per flag, cid_of."""
import datetime as dt

import numpy as np
import pytest

from crawler_amd.config import CrawlerConfig
from crawler_amd.engine.gpu_stage import (FetchStage, SpillRing,
                                          channel_ranges, cid_of,
                                          comment_cap)
from crawler_amd.ops import gpu

UTC = dt.timezone.utc


def offsets(lens):
    lens = np.asarray(lens, dtype=np.int32)
    off = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))[:-1]
    return off.astype(np.int64), lens


def brute(line_off, line_len, counts):
    """Per channel: the union of its lines' byte ranges and its written
    lines; (0, 0, 0) for a channel without a line."""
    out, row = [], 0
    for n in counts:
        rows = range(row, row + n)
        row += n
        if not n:
            out.append((0, 0, 0))
            continue
        out.append((min(int(line_off[r]) for r in rows),
                    max(int(line_off[r]) + int(line_len[r]) for r in rows),
                    sum(1 for r in rows if line_len[r] > 0)))
    return out


def as_tuples(got):
    lo_k, hi_k, n_k = got
    return [(int(a), int(b), int(c)) for a, b, c in zip(lo_k, hi_k, n_k)]


@pytest.mark.parametrize("K,P,lens", [
    (1, 1, [7]),
    (1, 1, [0]),
    (3, 4, [5, 6, 7, 8, 9, 1, 2, 3, 4, 4, 4, 4]),
    # a channel's first row, its last row and all of its rows empty
    (3, 4, [0, 6, 7, 8, 9, 1, 2, 0, 0, 0, 0, 0]),
    (3, 4, [0, 0, 0, 0, 0, 3, 0, 2, 4, 0, 0, 0]),
])
def test_channel_ranges_unwindowed(K, P, lens):
    off, ln = offsets(lens)
    got = as_tuples(channel_ranges(off, ln, K, P))
    assert got == brute(off, ln, [P] * K)
    assert sum(n for _lo, _hi, n in got) == int((ln > 0).sum())


@pytest.mark.parametrize("kept,lens", [
    ([2, 0, 1], [8, 8, 9]),
    ([0, 3, 0], [4, 5, 6]),
    ([0, 0, 0], []),
    ([1], [3]),
    # a kept row without a line as the first and as the last of a channel
    ([2, 0, 1], [0, 8, 9]),
    ([2, 0, 1], [8, 0, 9]),
    ([0, 3, 0], [0, 5, 0]),
    ([2, 2], [3, 0, 0, 4]),
    ([1], [0]),
])
def test_channel_ranges_windowed(kept, lens):
    off, ln = offsets(lens)
    kept_k = np.array(kept, dtype=np.int64)
    got = as_tuples(channel_ranges(off, ln, len(kept), 64, kept_k))
    assert got == brute(off, ln, kept)
    assert len(got) == len(kept)
    assert sum(n for _lo, _hi, n in got) == int((ln > 0).sum())


class FakeSink:
    """Stands in for the state manager: hands out one ticket per batch and
    records every call."""

    def __init__(self):
        self.calls = []

    def store_post_lines_batch(self, items, buf, ticket=False):
        assert ticket
        t = "t%d" % sum(c[0] == "store" for c in self.calls)
        self.calls.append(("store", t))
        return t

    def wait_post_write(self, ticket):
        self.calls.append(("wait", ticket))

    def drain_post_writes(self):
        self.calls.append(("drain",))


def test_spill_ring_ticket_protocol():
    sm = FakeSink()
    ring = SpillRing(sm)
    waits = lambda: [c[1] for c in sm.calls if c[0] == "wait"]
    s0 = ring.claim()
    ring.submit(s0, [("a", 0, 1)], b"x")      # t0 on slot 0
    s1 = ring.claim()
    ring.submit(s1, [("b", 0, 1)], b"x")      # t1 on slot 1
    assert (s0, s1) == (0, 1)
    assert waits() == [None, None]
    s2 = ring.claim()
    assert s2 == 0
    # exactly the ticket submitted on slot 0, and it is cleared
    assert waits() == [None, None, "t0"]
    ring.wait(0)
    assert waits()[-1] is None
    ring.submit(s2, [("c", 0, 1)], b"x")      # t2 on slot 0
    del sm.calls[:]
    ring.drain()
    assert sm.calls == [("wait", "t2"), ("wait", "t1"), ("drain",)]
    del sm.calls[:]
    ring.drain()
    assert sm.calls == [("wait", None), ("wait", None), ("drain",)]


def ts(x):
    return dt.datetime.fromtimestamp(x, UTC)


PLAN_CASES = {
    # flags -> (window at force_window=False, gate, cap)
    "none": ({}, False, False, False),
    "max-comments": ({"max_comments": 2}, False, False, True),
    "min-post-date": ({"min_post_date": ts(1700000000)}, False, False,
                      False),
    "max-posts": ({"max_posts": 9}, True, False, False),
    "date-between": ({"date_between_min": ts(1700060000),
                      "date_between_max": ts(1700089999)}, True, False,
                     False),
    "post-recency": ({"post_recency": ts(1700000000.5)}, True, True, False),
}


@pytest.mark.parametrize("as_walk", [False, True])
@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_fetch_stage_plan(case, as_walk):
    kw, window, gate, cap = PLAN_CASES[case]
    cfg = CrawlerConfig(crawl_id="s1", **kw)
    force = as_walk and (cfg.min_post_date is not None
                         or comment_cap(cfg) is not None)
    assert force == (as_walk and case in ("max-comments", "min-post-date"))
    stage = FetchStage(gpu, cfg, force_window=force)
    assert (stage.window is not None) == (window or force)
    assert (stage.gate is not None) == gate
    assert (stage.max_comments is not None) == cap
    assert stage.window == gpu.window_params(cfg, force=force or gate)
    assert stage.gate == gpu.gate_params(cfg)
    if cap:
        assert stage.max_comments == 2
    if case == "post-recency":
        # forced by the gate alone: the walk without bounds
        assert stage.window["stop_below"] is None
        assert stage.window["cap"] == 0


def test_comment_cap_none_and_negative():
    assert comment_cap(CrawlerConfig(crawl_id="s1")) is None
    assert comment_cap(CrawlerConfig(crawl_id="s1", max_comments=-5)) is None
    assert comment_cap(CrawlerConfig(crawl_id="s1", max_comments=0)) == 0


@pytest.mark.parametrize("name,universe,want", [
    ("c0000000007", 500, 7),
    ("c7", 500, 7),
    ("c0000000000", 500, 0),
    ("c0000000499", 500, 499),
    ("c0000000500", 500, None),
    ("c", 500, None),
    ("", 500, None),
    ("c12a", 500, None),
    ("x0000000007", 500, None),
    ("C0000000007", 500, None),
    ("c-1", 500, None),
])
def test_cid_of(name, universe, want):
    assert cid_of(name, universe) == want
