"""The channel gate (--time-ago), the kept-row compaction and the comment
cap (--max-comments) without a GPU: the oracle against the CPU crawl's
fetch_channel_messages + is_channel_active, the clamped batch against
run_for_channel's bytes, and the host half of the gated random walk."""
import datetime as dt
import random

import numpy as np
import pytest

from _gate_cases import (
    HAND_CASES,
    HAND_DATE,
    HAND_K,
    HAND_MSG,
    HAND_P,
    split_channels,
)
from crawler_amd.config import CrawlerConfig
from crawler_amd.engine import LocalStateManager, Page, RandomWalkStore
from crawler_amd.engine.pipeline import (
    fetch_channel_messages,
    is_channel_active,
    run_for_channel,
)
from crawler_amd.feed import FeedConfig, SyntheticFeed
from crawler_amd.feed.client import SyntheticTelegramClient
from crawler_amd.ops import golden_gate as GG
from crawler_amd.ops import golden_window as GW
from crawler_amd.ops import gpu
from crawler_amd.ops.golden_batch import encode_batch

UTC = dt.timezone.utc
NOW = dt.datetime(2026, 1, 2, tzinfo=UTC)
P = 64


def ts(x):
    return dt.datetime.fromtimestamp(x, UTC)


def mk_feed(**kw):
    return SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P, **kw))


def mk_cfg(tmp_path=None, **kw):
    kw.setdefault("sampling_method", "channel")
    return CrawlerConfig(crawl_id="gate1",
                         storage_root=str(tmp_path or "/nonexistent"),
                         min_users=1, **kw)


_batches = {}


def batch_of(feed, cids):
    key = (repr(feed.cfg), tuple(cids))
    if key not in _batches:
        _batches[key] = feed.build_batch(np.array(cids),
                                         posts_per_channel=P)
    return _batches[key]


def cpu_decision(client, feed, cfg, cid):
    """(fetched msg_ids, latest_ts, active) the way run_for_channel
    decides them."""
    info = client.search_public_chat(feed.username_of(cid))
    messages = fetch_channel_messages(client, info.chat_id, cfg,
                                      random.Random(0))
    latest = None
    if messages:
        latest = max(m.date for m in messages)
    else:
        newest = client.get_chat_history(info.chat_id, from_message_id=0,
                                         limit=1)
        if newest:
            latest = newest[0].date
    sg = client.get_supergroup_info(info.chat_id)
    active, _why = is_channel_active(latest, sg["member_count"], cfg,
                                     info.message_count)
    return {m.msg_id for m in messages}, latest, active


def oracle_decision(feed, cfg, cids):
    b = batch_of(feed, cids)
    date, msg = b.meta["date"].numpy(), b.msg_id.numpy()
    K = len(cids)
    keep, kept = GW.fetch_window(date, b.chat_id.numpy(), msg, P, K,
                                 **gpu.window_params(cfg, force=True))
    keep, kept, active, latest = GG.channel_gate(
        date, msg, P, K, gpu.gate_params(cfg)["recency"], keep, kept)
    return b, keep.reshape(K, P), kept, active, latest


@pytest.mark.parametrize("extra", [
    {},
    {"max_posts": 5},
    {"window": (40, P)},
    {"window": (10, 30)},
    {"min_post_date_at": 50},
], ids=["recency-only", "max-posts", "window-newest", "window-old",
        "min-post-date"])
def test_oracle_agrees_with_the_cpu_path(extra):
    feed = mk_feed()
    cids, cutoff, tie_cid = split_channels(feed, P)
    kw = {"post_recency": ts(cutoff)}
    c = feed.cfg
    if "max_posts" in extra:
        kw["max_posts"] = extra["max_posts"]
    if "window" in extra:
        first, last = extra["window"]
        kw["date_between_min"] = ts(c.base_date + first * c.date_step)
        kw["date_between_max"] = ts(c.base_date + last * c.date_step - 1)
    if "min_post_date_at" in extra:
        kw["min_post_date"] = ts(c.base_date
                                 + extra["min_post_date_at"] * c.date_step)
    cfg = mk_cfg(**kw)
    b, keep, kept, active, latest = oracle_decision(feed, cfg, cids)
    client = SyntheticTelegramClient(feed, posts_per_channel=P)
    msg = b.msg_id.numpy().reshape(len(cids), P)
    cpu_active = []
    for k, cid in enumerate(cids):
        ids, cpu_latest, act = cpu_decision(client, feed, cfg, cid)
        cpu_active.append(act)
        assert int(latest[k]) == cpu_latest, f"channel {cid} latest"
        assert bool(active[k]) == act, f"channel {cid} active"
        want = ids if act else set()
        assert set(msg[k][keep[k] != 0].tolist()) == want, f"channel {cid}"
        assert int(kept[k]) == len(want)
    if "window" in extra and extra["window"][1] < P:
        # the window ends before the band: everything fetched is older
        assert not any(cpu_active)
        return
    # the split is non-trivial, and the tie is on the inactive side
    assert any(cpu_active) and not all(cpu_active)
    assert not cpu_active[cids.index(tie_cid)]
    assert int(latest[cids.index(tie_cid)]) == cutoff


def test_a_fractional_cutoff_is_floored():
    feed = mk_feed()
    cids, cutoff, tie_cid = split_channels(feed, P)
    k = cids.index(tie_cid)
    client = SyntheticTelegramClient(feed, posts_per_channel=P)
    # just below the newest date: later than the cutoff, so active
    cfg = mk_cfg(post_recency=ts(cutoff - 0.5))
    assert gpu.gate_params(cfg) == {"recency": cutoff - 1}
    _b, _keep, kept, active, _latest = oracle_decision(feed, cfg, cids)
    assert active[k] == 1 and kept[k] == P
    assert cpu_decision(client, feed, cfg, tie_cid)[2] is True
    # just above it: inactive
    cfg = mk_cfg(post_recency=ts(cutoff + 0.5))
    assert gpu.gate_params(cfg) == {"recency": cutoff}
    _b, _keep, kept, active, _latest = oracle_decision(feed, cfg, cids)
    assert active[k] == 0 and kept[k] == 0
    assert cpu_decision(client, feed, cfg, tie_cid)[2] is False


def test_gate_params_and_forced_window_params():
    cfg = mk_cfg()
    assert gpu.gate_params(cfg) is None
    assert gpu.window_params(cfg) is None
    assert gpu.window_params(cfg, force=True) == {
        "stop_below": None, "skip_above": None, "cap": 0, "sample_k": 0,
        "seed": 0}
    cfg = mk_cfg(min_post_date=ts(1_700_000_100.5))
    assert gpu.window_params(cfg) is None
    forced = gpu.window_params(cfg, force=True)
    assert forced["stop_below"] == 1_700_000_101
    assert forced["skip_above"] is None
    # with a window configured, force changes nothing
    cfg = mk_cfg(max_posts=3)
    assert gpu.window_params(cfg, force=True) == gpu.window_params(cfg)


@pytest.mark.parametrize("recent", [True, False])
def test_empty_fetch_falls_back_to_the_newest_message(recent):
    feed = mk_feed()
    cids = [3, 9, 17]
    c = feed.cfg
    newest = batch_of(feed, cids).meta["date"].numpy().reshape(3, P).max(1)
    cutoff = int(newest.min()) - 1 if recent else int(newest.max())
    # a window that ends before the first post: nothing is fetched
    cfg = mk_cfg(date_between_min=ts(c.base_date - 1000),
                 date_between_max=ts(c.base_date - 500),
                 post_recency=ts(cutoff))
    b, keep, kept, active, latest = oracle_decision(feed, cfg, cids)
    assert kept.tolist() == [0, 0, 0] and not keep.any()
    assert latest.tolist() == newest.tolist()
    assert active.tolist() == [int(recent)] * 3
    client = SyntheticTelegramClient(feed, posts_per_channel=P)
    for k, cid in enumerate(cids):
        ids, cpu_latest, act = cpu_decision(client, feed, cfg, cid)
        assert ids == set() and cpu_latest == int(latest[k])
        assert act is recent


@pytest.mark.parametrize("keep,recency,want_active,want_latest", HAND_CASES)
def test_hand_built_arrays(keep, recency, want_active, want_latest):
    keep = np.array(keep, dtype=np.uint8)
    kept = keep.reshape(HAND_K, HAND_P).sum(1).astype(np.int32)
    before = keep.copy()
    k2, n2, active, latest = GG.channel_gate(
        HAND_DATE, HAND_MSG, HAND_P, HAND_K, recency, keep, kept)
    assert (keep == before).all(), "the oracle changed its input"
    assert active.tolist() == want_active
    assert latest.tolist() == want_latest
    for c in range(HAND_K):
        s = slice(c * HAND_P, (c + 1) * HAND_P)
        if want_active[c]:
            assert (k2[s] == before[s]).all() and n2[c] == kept[c]
        else:
            assert not k2[s].any() and n2[c] == 0


def test_compact_rows_oracle():
    rng = np.random.default_rng(4)
    K, Pn = 7, 70
    keep = (rng.random(K * Pn) < 0.3).astype(np.uint8)
    keep[2 * Pn:3 * Pn] = 0          # a channel without rows
    keep[5 * Pn:6 * Pn] = 1          # a full one
    kept = keep.reshape(K, Pn).sum(1).astype(np.int32)
    rows, chan = GG.compact_rows(keep, kept, Pn, K)
    assert rows.dtype == np.int64 and chan.dtype == np.int32
    assert rows.tolist() == np.flatnonzero(keep).tolist()
    assert chan.tolist() == (rows // Pn).tolist()
    for c in range(K):
        mine = rows[chan == c]
        assert (np.diff(mine) > 0).all() and len(mine) == kept[c]
    # nothing kept anywhere
    rows, chan = GG.compact_rows(np.zeros(K * Pn, np.uint8),
                                 np.zeros(K, np.int32), Pn, K)
    assert rows.shape == (0,) and chan.shape == (0,)
    assert rows.dtype == np.int64 and chan.dtype == np.int32
    rows, chan = GG.compact_rows(np.zeros(0, np.uint8),
                                 np.zeros(0, np.int32), Pn, 0)
    assert rows.size == 0 and chan.size == 0


# ---- comment cap ----

COM_CIDS = [3, 9]


def com_feed():
    return mk_feed(comment_rate=0.5, max_comments_per_post=3)


def test_comment_feed_precondition():
    b = batch_of(com_feed(), COM_CIDS)
    cnt = b.meta["com_cnt"].numpy()
    assert (b.meta["reply_count"].numpy() == cnt).all()
    assert (cnt == 3).any() and (cnt == 1).any() and (cnt == 0).any()


@pytest.mark.parametrize("max_comments", [0, 1, 2, 3, -1])
def test_comment_cap_matches_run_for_channel(tmp_path, max_comments):
    feed = com_feed()
    cfg = mk_cfg(tmp_path, max_comments=max_comments)
    b = batch_of(feed, COM_CIDS)
    capped = gpu.cap_comments(b, max_comments)
    if max_comments < 0:
        assert capped is b
    else:
        assert capped is not b
        assert (capped.meta["com_cnt"].numpy()
                == np.minimum(b.meta["com_cnt"].numpy(),
                              max_comments)).all()
        # the column is a copy and the comment table is shared
        assert capped.com_text_off is b.com_text_off
    before = b.meta["com_cnt"].clone()
    lines, _links = encode_batch(capped, now=NOW)
    assert (b.meta["com_cnt"] == before).all()
    sm = LocalStateManager(cfg)
    client = SyntheticTelegramClient(feed, posts_per_channel=P)
    for cid in COM_CIDS:
        res = run_for_channel(client, Page(id="p%d" % cid,
                                           url=feed.username_of(cid)),
                              sm, cfg, rng=random.Random(0), now=NOW)
        assert res.status == "fetched" and res.posts_stored == P
    sm.close()
    for k, cid in enumerate(COM_CIDS):
        path = (tmp_path / "gate1" / feed.username_of(cid) / "posts"
                / "posts.jsonl")
        # run_for_channel writes newest first, the batch is oldest first
        want = b"".join(reversed(lines[k * P:(k + 1) * P]))
        assert path.read_bytes() == want, f"channel {cid}"


# ---- host half of the gated random walk ----

def mk_walk(tmp_path):
    from crawler_amd.engine.gpu_randomwalk import GpuRandomWalk
    from crawler_amd.engine.gpu_stage import SpillRing
    import collections

    cfg = CrawlerConfig(crawl_id="gw1", storage_root=str(tmp_path),
                        sampling_method="random-walk", min_users=1,
                        walkback_rate=0)
    g = GpuRandomWalk.__new__(GpuRandomWalk)
    g.cfg = cfg
    g.sm = LocalStateManager(cfg)
    g.rw = RandomWalkStore()
    g.rng = random.Random(5)
    g.ppc = P
    g.stats = {"pages": 0, "posts": 0, "invalid_400": 0,
               "walkback_exhausted": 0, "edges": 0, "deadends": 0}
    g.timings = collections.defaultdict(float)
    g.spill = SpillRing(g.sm)
    g._inflight_paths = {}
    g._vc_init(1 << 8)
    for i in range(100, 130):
        g.sm.add_discovered_channel("c%010d" % i)
    live = [Page(id="p%d" % i, url="c%010d" % i, depth=0,
                 sequence_id="sq%d" % i, status="unfetched")
            for i in range(3)]
    for p in live:
        g.rw.add_page(p)
    return g, live


def test_walk_host_deadend_and_zero_row_walkers(tmp_path):
    """Walker 0 is active without a kept row, walker 1 is inactive,
    walker 2 is active without a kept row: nothing was encoded."""
    from crawler_amd.engine.gpu_randomwalk import GpuRandomWalk

    g, live = mk_walk(tmp_path)
    payload = GpuRandomWalk._empty_payload(
        0, NOW, np.zeros(3, dtype=np.int64),
        np.array([True, False, True]))
    g._hop_host(live, payload)
    g.sm.close()
    assert g.stats["pages"] == 3 and g.stats["deadends"] == 1
    assert g.stats["posts"] == 0
    assert not list(tmp_path.rglob("posts.jsonl"))
    for p in live:
        assert p.id not in g.rw.page_buffer
    children = {p.parent_id: p for p in g.rw.page_buffer.values()}
    assert set(children) == {"p0", "p2"}
    edges = g.rw.edge_records
    assert {e.source_channel for e in edges} == {live[0].url, live[2].url}
    # without a link every active walker walks back, on a fresh chain
    assert all(e.walkback and not e.skipped for e in edges)
    assert children["p0"].sequence_id != live[0].sequence_id
    assert g.rw.get_channel_last_crawled(live[1].url) is not None


def test_walk_host_windowed_ranges(tmp_path):
    """Walker 0 owns two lines and one link, walker 1 is inactive, walker
    2 owns one line and no link: ranges come from the cumsum of kept and
    the link's walker from the payload, not from row // P."""
    import torch

    g, live = mk_walk(tmp_path)
    blob = b'{"a":0}\n{"a":1}\n{"b":22}\n'
    name = np.zeros((1, 32), dtype=np.uint8)
    name[0, :11] = np.frombuffer(b"c0000000200", dtype=np.uint8)
    payload = {
        "slot": 0, "ev": None, "res_out": None,
        "out_host": torch.frombuffer(bytearray(blob), dtype=torch.uint8),
        "line_off": np.array([0, 8, 16], dtype=np.int64),
        "line_len": np.array([8, 8, 9], dtype=np.int32),
        "u_w": np.array([0], dtype=np.int32),
        "u_h": np.array([gpu.fnv1a64(b"c0000000200")],
                        dtype=np.uint64).view(np.int64),
        "u_rows": name, "ok_all": np.array([True]),
        "cid_ok_all": np.array([True]), "w": 32, "now": NOW,
        "kept_k": np.array([2, 0, 1], dtype=np.int64),
        "active_k": np.array([True, False, True]),
    }
    g._hop_host(live, payload)
    g.spill.drain()
    g.sm.close()
    read = lambda p: (tmp_path / "gw1" / p.url / "posts"
                      / "posts.jsonl")
    assert read(live[0]).read_bytes() == blob[:16]
    assert not read(live[1]).exists()
    assert read(live[2]).read_bytes() == blob[16:]
    assert g.stats["posts"] == 3 and g.stats["pages"] == 3
    assert g.stats["deadends"] == 1
    children = {p.parent_id: p for p in g.rw.page_buffer.values()}
    assert set(children) == {"p0", "p2"}
    # walkback_rate 0: walker 0 follows its only link, on its own chain
    assert children["p0"].url == "c0000000200"
    assert children["p0"].sequence_id == live[0].sequence_id
    by_src = {e.source_channel: e for e in g.rw.edge_records}
    assert set(by_src) == {live[0].url, live[2].url}
    assert not by_src[live[0].url].walkback
    assert by_src[live[2].url].walkback
