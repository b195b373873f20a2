"""The GPU random walk with the fetch and deadend flags (--date-between,
--min-post-date, --time-ago, --max-comments): one hop over n seeds against
the window and gate oracles and the golden encoder, the unchanged launches
of a walk without a flag, and the CLI end to end on both GPU engines."""
import datetime as dt
import json
import random

import numpy as np
import pytest

from _gate_cases import split_channels
from crawler_amd.config import CrawlerConfig
from crawler_amd.engine import LocalStateManager, RandomWalkStore
from crawler_amd.feed import FeedConfig, SyntheticFeed
from crawler_amd.ops import golden_gate as GG
from crawler_amd.ops import golden_window as GW
from crawler_amd.ops.golden_batch import encode_batch

pytestmark = pytest.mark.gpu

UTC = dt.timezone.utc
NOW = dt.datetime(2026, 1, 1, tzinfo=UTC)
P = 64
CIDS = [1, 2, 3, 5, 8, 13]
NEW_ENTRY_POINTS = {"crawl_fetch_window", "crawl_channel_gate",
                    "crawl_compact_rows"}


def ts(x):
    return dt.datetime.fromtimestamp(x, UTC)


def mk_feed(**kw):
    return SyntheticFeed(FeedConfig(seed=44, universe=500,
                                    posts_per_channel=P, **kw))


def mk(tmp_path, feed, **kw):
    from crawler_amd.engine.gpu_randomwalk import GpuRandomWalk

    kw.setdefault("walkback_rate", 15)
    cfg = CrawlerConfig(crawl_id="grw1", storage_root=str(tmp_path),
                        sampling_method="random-walk", min_users=1, **kw)
    sm = LocalStateManager(cfg)
    rw = RandomWalkStore()
    eng = GpuRandomWalk(cfg, sm, rw, feed, posts_per_hop=P, walkers=16,
                        rng=random.Random(3))
    return cfg, sm, rw, eng


_golden = {}


def golden(feed, cids, max_comments=-1):
    from crawler_amd.ops import gpu

    key = (repr(feed.cfg), tuple(cids), max_comments)
    if key not in _golden:
        b = feed.build_batch(np.array(cids), posts_per_channel=P)
        _golden[key] = (b,) + encode_batch(gpu.cap_comments(b, max_comments),
                                           now=NOW)
    return _golden[key]


def expectation(feed, cfg, cids):
    """Per channel: the expected posts.jsonl bytes, the link names of its
    kept rows, and whether it is active."""
    from crawler_amd.ops import gpu

    b, lines, links = golden(feed, cids, cfg.max_comments)
    K = len(cids)
    date, msg = b.meta["date"].numpy(), b.msg_id.numpy()
    keep, kept = GW.fetch_window(date, b.chat_id.numpy(), msg, P, K,
                                 **gpu.window_params(cfg, force=True))
    active = np.ones(K, dtype=np.uint8)
    gate = gpu.gate_params(cfg)
    if gate is not None:
        keep, kept, active, _ = GG.channel_gate(date, msg, P, K,
                                                gate["recency"], keep, kept)
    files, names = [], []
    for k in range(K):
        rows = [k * P + r for r in range(P) if keep[k * P + r]]
        files.append(b"".join(lines[r] for r in rows))
        names.append({n for r in rows for (n, _s) in links[r]})
    return files, names, active


def one_hop(tmp_path, feed, cids, pipelined=False, **kw):
    """Seed the channels, run exactly one hop, and check files, edges and
    child pages against the expectation."""
    cfg, sm, rw, eng = mk(tmp_path, feed, **kw)
    names = ["c%010d" % c for c in cids]
    eng.seed(names)
    page_of = {p.url: p.id for p in rw.page_buffer.values()}
    assert set(page_of) == set(names)
    stats = eng.run(max_pages=len(cids), now=NOW, pipelined=pipelined)
    files, link_names, active = expectation(feed, cfg, cids)
    assert stats["pages"] == len(cids)
    assert stats["deadends"] == int((active == 0).sum())
    assert stats["posts"] == sum(f.count(b"\n") for f in files)
    children = {p.parent_id for p in rw.page_buffer.values()}
    edges = rw.edge_records
    for k, name in enumerate(names):
        path = tmp_path / "grw1" / name / "posts" / "posts.jsonl"
        mine = [e for e in edges if e.source_channel == name]
        assert page_of[name] not in rw.page_buffer
        if not active[k]:
            assert not path.exists(), f"deadend {name} wrote a file"
            assert mine == [] and page_of[name] not in children
            continue
        if files[k]:
            assert path.read_bytes() == files[k], f"{name} JSONL differs"
        else:
            assert not path.exists(), f"{name}: a file for no post"
        assert page_of[name] in children
        followed = [e for e in mine if not e.skipped]
        assert len(followed) == 1
        for e in mine:
            if e.walkback:
                continue
            # followed or skipped: linked from a kept row of its source
            assert e.destination_channel in link_names[k], (name, e)
        if not link_names[k]:
            assert followed[0].walkback and len(mine) == 1
    return cfg, rw, eng, files, link_names, active


def window_kw(feed, first, last):
    c = feed.cfg
    return dict(date_between_min=ts(c.base_date + first * c.date_step),
                date_between_max=ts(c.base_date + last * c.date_step - 1))


@pytest.mark.parametrize("pipelined", [False, True])
def test_date_window(tmp_path, pipelined):
    feed = mk_feed()
    cfg, rw, eng, files, link_names, active = one_hop(
        tmp_path, feed, CIDS, pipelined, **window_kw(feed, 16, 48))
    assert [f.count(b"\n") for f in files] == [32] * len(CIDS)
    assert active.all()
    # the window does hide links: the whole channel has more
    _b, _lines, links = golden(feed, CIDS)
    whole = {n for row in links[:P] for (n, _s) in row}
    assert link_names[0] < whole
    assert any(not e.walkback and not e.skipped for e in rw.edge_records)


def test_min_post_date_only(tmp_path):
    feed = mk_feed()
    lo = feed.cfg.base_date + 40 * feed.cfg.date_step
    cfg, rw, eng, files, _names, _active = one_hop(
        tmp_path, feed, CIDS, min_post_date=ts(lo))
    assert [f.count(b"\n") for f in files] == [P - 40] * len(CIDS)


def test_window_with_max_posts_and_sample(tmp_path):
    feed = mk_feed()
    cfg, rw, eng, files, _names, _active = one_hop(
        tmp_path, feed, CIDS, max_posts=20, sample_size=5, sample_seed=4,
        **window_kw(feed, 10, 50))
    assert [f.count(b"\n") for f in files] == [5] * len(CIDS)


def test_post_recency_splits_the_seeds(tmp_path):
    feed = mk_feed()
    cids, cutoff, tie_cid = split_channels(feed, P)
    cfg, rw, eng, files, _names, active = one_hop(
        tmp_path, feed, cids, post_recency=ts(cutoff))
    assert active.any() and not active.all()
    assert not active[cids.index(tie_cid)]
    assert [f.count(b"\n") for f in files] == [P * int(a) for a in active]


def test_a_window_without_posts_walks_every_walker_back(tmp_path,
                                                        monkeypatch):
    from crawler_amd.ops import gpu

    feed = mk_feed()
    real, launched = gpu._call, []

    def spy(name, *args, **kwargs):
        launched.append(name)
        return real(name, *args, **kwargs)

    monkeypatch.setattr(gpu, "_call", spy)
    c = feed.cfg
    cfg, rw, eng, files, link_names, active = one_hop(
        tmp_path, feed, CIDS,
        date_between_min=ts(c.base_date - 1000),
        date_between_max=ts(c.base_date - 500),
        post_recency=ts(c.base_date))
    assert active.all() and files == [b""] * len(CIDS)
    assert not list(tmp_path.rglob("posts.jsonl"))
    assert len(rw.edge_records) == len(CIDS)
    assert all(e.walkback for e in rw.edge_records)
    # nothing to encode, claim or compact
    assert "crawl_fetch_window" in launched
    assert "crawl_channel_gate" in launched
    assert "crawl_measure_extract" not in launched
    assert "crawl_claim_links" not in launched
    assert "crawl_compact_rows" not in launched


def test_max_comments_in_the_walk(tmp_path):
    feed = mk_feed(comment_rate=0.5, max_comments_per_post=3)
    b, _lines, _links = golden(feed, CIDS)
    assert (b.meta["com_cnt"].numpy() == 3).any()
    cfg, rw, eng, files, _names, _active = one_hop(
        tmp_path, feed, CIDS, max_comments=1)
    for f in files:
        n_com = [len(json.loads(l)["comments"]) for l in f.splitlines()]
        assert len(n_com) == P and max(n_com) == 1


def test_without_a_flag_nothing_new_is_launched(tmp_path, monkeypatch):
    from crawler_amd.ops import gpu

    feed = mk_feed()
    real, launched = gpu._call, []

    def spy(name, *args, **kwargs):
        launched.append(name)
        return real(name, *args, **kwargs)

    monkeypatch.setattr(gpu, "_call", spy)
    cfg, sm, rw, eng = mk(tmp_path, feed)
    assert (eng.fetch.window is None and eng.fetch.gate is None
            and eng.fetch.max_comments is None)
    names = ["c%010d" % c for c in CIDS]
    eng.seed(names)
    stats = eng.run(max_pages=len(CIDS), now=NOW)
    assert "crawl_measure_extract" in launched
    assert not NEW_ENTRY_POINTS & set(launched)
    assert stats["pages"] == len(CIDS) and stats["deadends"] == 0
    assert stats["posts"] == len(CIDS) * P
    _b, lines, _links = golden(feed, CIDS)
    for k, name in enumerate(names):
        path = tmp_path / "grw1" / name / "posts" / "posts.jsonl"
        assert path.read_bytes() == b"".join(lines[k * P:(k + 1) * P])


# ---- CLI ----

def cli_channel(tmp_path, crawl_id, time_ago):
    from crawler_amd.cli import main

    rc = main([
        "--mode", "standalone", "--gpu", "--sampling", "channel",
        "--urls", "c0000000001,c0000000002,c0000000007",
        "--storage-root", str(tmp_path), "--crawl-id", crawl_id,
        "--synthetic-universe", "300", "--synthetic-posts", "32",
        "--time-ago", time_ago, "--min-users", "1", "--skip-media",
    ])
    assert rc == 0
    prog = json.loads((tmp_path / crawl_id / "progress.json").read_text())
    assert prog["status"] == "completed"
    return list((tmp_path / crawl_id).rglob("posts.jsonl"))


def test_cli_time_ago_one_day_deadends_every_page(tmp_path):
    # the synthetic posts are from 2023
    assert cli_channel(tmp_path, "gago1", "1d") == []


def test_cli_time_ago_fifty_years_keeps_everything(tmp_path):
    jsonls = cli_channel(tmp_path, "gago2", "50y")
    assert len(jsonls) == 3
    for path in jsonls:
        assert path.read_bytes().count(b"\n") == 32


def test_cli_random_walk_date_between_max_comments(tmp_path):
    from crawler_amd.cli import main

    base = FeedConfig().base_date
    day = dt.datetime.fromtimestamp(base, UTC).replace(
        hour=0, minute=0, second=0, microsecond=0)
    nxt = day + dt.timedelta(days=1)
    assert base + 255 * FeedConfig().date_step > nxt.timestamp()
    rc = main([
        "--mode", "standalone", "--gpu", "--sampling", "random-walk",
        "--seed-size", "8", "--max-pages", "16",
        "--storage-root", str(tmp_path), "--crawl-id", "gwalk2",
        "--synthetic-universe", "500", "--synthetic-posts", "256",
        "--date-between", "%s,%s" % (day.strftime("%Y-%m-%d"),
                                     nxt.strftime("%Y-%m-%d")),
        "--max-comments", "0",
        "--concurrency", "16", "--min-users", "1", "--skip-media",
    ])
    assert rc == 0
    jsonls = list((tmp_path / "gwalk2").rglob("posts.jsonl"))
    assert jsonls
    n = 0
    for path in jsonls:
        for line in path.read_bytes().splitlines():
            post = json.loads(line)
            at = dt.datetime.strptime(post["published_at"],
                                      "%Y-%m-%dT%H:%M:%SZ").replace(tzinfo=UTC)
            assert day <= at <= nxt
            assert post["comments"] == []
            n += 1
    assert n > 0
