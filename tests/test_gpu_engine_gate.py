"""The GPU crawl engine with --time-ago and --max-comments: the channel
gate against its oracle, the golden encoder and a StandaloneRunner crawl
of the same configuration; the comment cap against the clamped batch; and
the unchanged launches of a crawl without any of these flags."""
import datetime as dt
import json

import numpy as np
import pytest

from _gate_cases import split_channels
from crawler_amd.config import CrawlerConfig
from crawler_amd.engine import LocalStateManager
from crawler_amd.feed import FeedConfig, SyntheticFeed
from crawler_amd.ops import golden_gate as GG
from crawler_amd.ops import golden_window as GW
from crawler_amd.ops.golden_batch import encode_batch

pytestmark = pytest.mark.gpu

UTC = dt.timezone.utc
NOW = dt.datetime(2026, 1, 2, tzinfo=UTC)
P = 64
NEW_ENTRY_POINTS = {"crawl_fetch_window", "crawl_channel_gate",
                    "crawl_compact_rows"}


def ts(x):
    return dt.datetime.fromtimestamp(x, UTC)


def mk_feed(**kw):
    return SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P, **kw))


def mk_engine(tmp_path, feed, crawl_id="g1", chunk_channels=256, **cfg_kw):
    from crawler_amd.engine.gpu_runner import GpuCrawlEngine

    cfg_kw.setdefault("sampling_method", "channel")
    cfg = CrawlerConfig(crawl_id=crawl_id, storage_root=str(tmp_path),
                        min_users=1, **cfg_kw)
    sm = LocalStateManager(cfg)
    eng = GpuCrawlEngine(cfg, sm, feed, posts_per_channel=P,
                         chunk_channels=chunk_channels, fixed_now=NOW)
    return cfg, sm, eng


_golden = {}


def golden(feed, cids, max_comments=-1):
    """(cpu batch, lines, links) of the channels at NOW, computed once."""
    from crawler_amd.ops import gpu

    key = (repr(feed.cfg), tuple(cids), max_comments)
    if key not in _golden:
        b = feed.build_batch(np.array(cids), posts_per_channel=P)
        _golden[key] = (b,) + encode_batch(gpu.cap_comments(b, max_comments),
                                           now=NOW)
    return _golden[key]


def expectation(feed, cfg, cids):
    """Per channel the expected posts.jsonl bytes (b"" = no file), the
    links of the kept rows of the active channels, and the oracle's
    active flags (all ones without --time-ago)."""
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
    files, names = [], set()
    for k in range(K):
        rows = [k * P + r for r in range(P) if keep[k * P + r]]
        files.append(b"".join(lines[r] for r in rows))
        names |= {n for r in rows for (n, _s) in links[r]}
    return files, names, active


def read_posts(tmp_path, crawl_id, cid):
    path = tmp_path / crawl_id / ("c%010d" % cid) / "posts" / "posts.jsonl"
    return path.read_bytes() if path.exists() else None


def window_kw(feed, first, last):
    c = feed.cfg
    return dict(date_between_min=ts(c.base_date + first * c.date_step),
                date_between_max=ts(c.base_date + last * c.date_step - 1))


@pytest.mark.parametrize("chunk_channels", [1, 4, 256])
@pytest.mark.parametrize("extra", ["recency-only", "window-max-posts",
                                   "min-post-date"])
def test_post_recency_splits_the_channels(tmp_path, extra, chunk_channels):
    feed = mk_feed()
    cids, cutoff, tie_cid = split_channels(feed, P)
    kw = {"post_recency": ts(cutoff)}
    if extra == "window-max-posts":
        kw.update(window_kw(feed, 40, P), max_posts=9)
    elif extra == "min-post-date":
        kw["min_post_date"] = ts(feed.cfg.base_date
                                 + 50 * feed.cfg.date_step)
    cfg, sm, eng = mk_engine(tmp_path, feed, "g1", chunk_channels, **kw)
    names = ["c%010d" % c for c in cids]
    discovered, posts = eng.process_channels(names, now=NOW)
    sm.close()
    files, link_names, active = expectation(feed, cfg, cids)
    assert active.any() and not active.all()
    assert not active[cids.index(tie_cid)], "a tie is inactive"
    dead = {names[k] for k in range(len(cids)) if not active[k]}
    assert eng.last_deadends == dead
    assert eng.stats["deadends"] == len(dead)
    for k, cid in enumerate(cids):
        got = read_posts(tmp_path, "g1", cid)
        if not active[k]:
            assert got is None, f"deadend channel {cid} wrote a file"
            assert files[k] == b""
        else:
            assert files[k] and got == files[k], f"channel {cid} JSONL"
    assert set(discovered) == link_names
    n_lines = sum(f.count(b"\n") for f in files)
    assert posts == n_lines and eng.stats["posts"] == n_lines
    assert eng.stats["pages"] == len(cids)


def test_every_channel_inactive_records_the_deadends(tmp_path):
    """The chunk keeps nothing, so it leaves through the early exit."""
    feed = mk_feed()
    cids = [3, 9, 17]
    cfg, sm, eng = mk_engine(tmp_path, feed,
                             post_recency=dt.datetime(2025, 1, 1,
                                                      tzinfo=UTC))
    names = ["c%010d" % c for c in cids]
    discovered, posts = eng.process_channels(names, now=NOW)
    sm.close()
    assert eng.last_deadends == set(names) and eng.stats["deadends"] == 3
    assert posts == 0 and list(discovered) == []
    assert eng.stats["pages"] == 3
    assert not list(tmp_path.rglob("posts.jsonl"))


def cpu_crawl(tmp_path, feed, names, **cfg_kw):
    """A StandaloneRunner crawl of the same configuration at NOW."""
    from crawler_amd.engine import pipeline
    from crawler_amd.engine.runner import StandaloneRunner
    from crawler_amd.feed.client import ConnectionPool

    cfg = CrawlerConfig(crawl_id="g1", storage_root=str(tmp_path),
                        min_users=1, sampling_method="channel",
                        concurrency=1, disable_rate_limits=True, **cfg_kw)
    sm = LocalStateManager(cfg)
    pool = ConnectionPool(feed, 1, cfg.rate_limit, posts_per_channel=P,
                          disable_rate_limits=True)

    def at_now(pool, page, sm, cfg, **kw):
        return pipeline.run_for_channel_with_pool(pool, page, sm, cfg,
                                                  now=NOW, **kw)

    stats = StandaloneRunner(cfg, sm, pool, run_for_channel_fn=at_now).run(
        names, resume=False)
    return sm, stats


def test_run_marks_deadend_pages_and_matches_the_cpu_crawl(tmp_path):
    feed = mk_feed()
    cids, cutoff, _tie = split_channels(feed, P)
    names = ["c%010d" % c for c in cids]
    kw = dict(post_recency=ts(cutoff), max_posts=9)
    cfg, sm, eng = mk_engine(tmp_path / "gpu", feed, **kw)
    stats = eng.run(names, resume=False)
    _files, _links, active = expectation(feed, cfg, cids)
    status = {p.url: p.status for p in sm.pages.values()}
    assert status == {names[k]: ("fetched" if active[k] else "deadend")
                      for k in range(len(cids))}
    assert stats["deadends"] == int((active == 0).sum()) > 0
    prog = json.loads((tmp_path / "gpu" / "g1" / "progress.json")
                      .read_text())
    assert prog["status"] == "completed"

    cpu_sm, cpu_stats = cpu_crawl(tmp_path / "cpu", feed, names, **kw)
    assert {p.url: p.status for p in cpu_sm.pages.values()} == status
    assert cpu_stats["deadends"] == stats["deadends"]
    assert cpu_stats["posts"] == stats["posts"]
    written = lambda root: sorted(
        str(p.relative_to(root)) for p in root.rglob("posts.jsonl"))
    assert written(tmp_path / "gpu") == written(tmp_path / "cpu")
    assert len(written(tmp_path / "gpu")) == int(active.sum())
    for k, cid in enumerate(cids):
        got = read_posts(tmp_path / "gpu", "g1", cid)
        cpu = read_posts(tmp_path / "cpu", "g1", cid)
        if not active[k]:
            assert got is None and cpu is None
            continue
        # the same lines; the CPU crawl writes a channel newest first,
        # the GPU crawl oldest first
        assert got.splitlines()[::-1] == cpu.splitlines(), f"channel {cid}"


# ---- --max-comments ----

COM_CIDS = [3, 9, 17]


def com_feed():
    return mk_feed(comment_rate=0.5, max_comments_per_post=3)


@pytest.mark.parametrize("max_comments,windowed", [
    (0, False), (1, False), (-1, False), (1, True)])
def test_max_comments(tmp_path, monkeypatch, max_comments, windowed):
    from crawler_amd.ops import gpu

    feed = com_feed()
    b, _lines, _links = golden(feed, COM_CIDS)
    cnt = b.meta["com_cnt"].numpy()
    assert (cnt == 3).any() and (cnt == 1).any()
    kw = window_kw(feed, 16, 48) if windowed else {}
    real, launched = gpu._call, []

    def spy(name, *args, **kwargs):
        launched.append(name)
        return real(name, *args, **kwargs)

    monkeypatch.setattr(gpu, "_call", spy)
    cfg, sm, eng = mk_engine(tmp_path, feed, max_comments=max_comments,
                             **kw)
    names = ["c%010d" % c for c in COM_CIDS]
    discovered, posts = eng.process_channels(names, now=NOW)
    sm.close()
    assert ("crawl_fetch_window" in launched) == windowed
    assert "crawl_channel_gate" not in launched
    files, link_names, _active = expectation(feed, cfg, COM_CIDS)
    for k, cid in enumerate(COM_CIDS):
        got = read_posts(tmp_path, "g1", cid)
        assert got == files[k], f"channel {cid} JSONL differs"
        n_com = [len(json.loads(l)["comments"]) for l in got.splitlines()]
        if max_comments >= 0:
            assert max(n_com) == max_comments
        else:
            assert max(n_com) == 3
    assert set(discovered) == link_names
    assert posts == (3 * 32 if windowed else 3 * P)
    if max_comments < 0:
        # no cap: the bytes of a crawl without the flag
        plain = golden(feed, COM_CIDS)[1]
        assert b"".join(files) == b"".join(plain)


def test_without_a_flag_nothing_new_is_launched(tmp_path, monkeypatch):
    from crawler_amd.ops import gpu

    feed = mk_feed()
    cids = [3, 9, 17]
    real, launched = gpu._call, []

    def spy(name, *args, **kwargs):
        launched.append(name)
        return real(name, *args, **kwargs)

    monkeypatch.setattr(gpu, "_call", spy)
    cfg, sm, eng = mk_engine(tmp_path, feed, sampling_method="snowball",
                             max_depth=1)
    assert gpu.window_params(cfg) is None and gpu.gate_params(cfg) is None
    names = ["c%010d" % c for c in cids]
    discovered, posts = eng.process_channels(names, now=NOW)
    sm.close()
    assert "crawl_measure_extract" in launched
    assert not NEW_ENTRY_POINTS & set(launched)
    _b, lines, links = golden(feed, cids)
    for k, cid in enumerate(cids):
        assert read_posts(tmp_path, "g1", cid) == b"".join(
            lines[k * P:(k + 1) * P]), f"channel {cid} JSONL differs"
    assert set(discovered) == {n for row in links for (n, _s) in row}
    assert posts == 3 * P and eng.last_deadends == set()


def test_max_posts_alone_compacts_its_rows_on_the_device(tmp_path,
                                                         monkeypatch):
    """A window without a gate takes its kept rows from the compact-rows
    kernel too, over more than one chunk."""
    from crawler_amd.ops import gpu

    feed = mk_feed()
    cids, _cutoff, _tie = split_channels(feed, P)
    assert len(cids) == 6
    real, launched = gpu._call, []

    def spy(name, *args, **kwargs):
        launched.append(name)
        return real(name, *args, **kwargs)

    monkeypatch.setattr(gpu, "_call", spy)
    cfg, sm, eng = mk_engine(tmp_path, feed, chunk_channels=4, max_posts=9)
    assert gpu.gate_params(cfg) is None
    names = ["c%010d" % c for c in cids]
    discovered, posts = eng.process_channels(names, now=NOW)
    sm.close()
    assert launched.count("crawl_fetch_window") == 2
    assert launched.count("crawl_compact_rows") == 2
    assert "crawl_channel_gate" not in launched
    files, link_names, _active = expectation(feed, cfg, cids)
    for k, cid in enumerate(cids):
        assert files[k].count(b"\n") == 9
        assert read_posts(tmp_path, "g1", cid) == files[k], f"channel {cid}"
    assert set(discovered) == link_names
    assert posts == 6 * 9 and eng.stats["posts"] == 6 * 9
    assert eng.stats["pages"] == 6 and eng.last_deadends == set()
