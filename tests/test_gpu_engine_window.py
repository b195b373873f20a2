"""The GPU crawl engine with a fetch window: --date-between, --max-posts
and --sample-size against the oracle mask, the CPU crawl's
fetch_channel_messages and the golden encoder."""
import datetime as dt
import json

import numpy as np
import pytest

from crawler_amd.config import CrawlerConfig
from crawler_amd.engine import LocalStateManager
from crawler_amd.feed import FeedConfig, SyntheticFeed
from crawler_amd.ops import golden_window as GW
from crawler_amd.ops.golden_batch import encode_batch

pytestmark = pytest.mark.gpu

UTC = dt.timezone.utc
NOW = dt.datetime(2026, 1, 2, tzinfo=UTC)
P = 64
CIDS = [3, 9, 17]


def ts(x):
    return dt.datetime.fromtimestamp(x, UTC)


def mk_engine(tmp_path, crawl_id="w1", chunk_channels=256, **cfg_kw):
    from crawler_amd.engine.gpu_runner import GpuCrawlEngine

    cfg_kw.setdefault("sampling_method", "channel")
    cfg = CrawlerConfig(crawl_id=crawl_id, storage_root=str(tmp_path),
                        min_users=1, **cfg_kw)
    feed = SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P))
    sm = LocalStateManager(cfg)
    eng = GpuCrawlEngine(cfg, sm, feed, posts_per_channel=P,
                         chunk_channels=chunk_channels)
    return cfg, feed, sm, eng


def bounds(feed, first, last):
    """(lo, hi) that hold the posts ``first`` .. ``last`` - 1 of every
    channel: post p is dated base_date + p * date_step + (0 .. 29)."""
    c = feed.cfg
    assert c.date_step > 29
    return (c.base_date + first * c.date_step,
            c.base_date + last * c.date_step - 1)


_golden = {}


def golden(feed, cids, min_post_date=None):
    """(cpu batch, lines, links) of the channels, computed once."""
    key = (tuple(cids), min_post_date)
    if key not in _golden:
        b = feed.build_batch(np.array(cids), posts_per_channel=P)
        _golden[key] = (b,) + encode_batch(b, now=NOW,
                                           min_post_date=min_post_date)
    return _golden[key]


def expectation(feed, cfg, cids=CIDS):
    """Per channel the expected posts.jsonl bytes (b"" = no file), the
    kept rows' link names and the oracle's kept counts."""
    from crawler_amd.ops import gpu

    b, lines, links = golden(feed, cids, cfg.min_post_date)
    params = gpu.window_params(cfg)
    assert params is not None
    keep, kept = GW.fetch_window(b.meta["date"].numpy(), b.chat_id.numpy(),
                                 b.msg_id.numpy(), P, len(cids), **params)
    files, names = [], set()
    for k in range(len(cids)):
        rows = [k * P + r for r in range(P) if keep[k * P + r]]
        files.append(b"".join(lines[r] for r in rows))
        names |= {n for r in rows for (n, _s) in links[r]}
    return files, names, keep.reshape(len(cids), P), kept


def read_posts(tmp_path, crawl_id, cid):
    path = tmp_path / crawl_id / ("c%010d" % cid) / "posts" / "posts.jsonl"
    return path.read_bytes() if path.exists() else None


def msg_ids_of(data):
    """msg_ids of a posts.jsonl: post_uid is '<msg_id >> 20>-<username>'."""
    return {int(json.loads(l)["post_uid"].split("-")[0]) << 20
            for l in data.splitlines()}


def cpu_fetch_ids(feed, cfg, cid):
    from crawler_amd.engine.pipeline import fetch_channel_messages
    from crawler_amd.feed.client import SyntheticTelegramClient

    client = SyntheticTelegramClient(feed, posts_per_channel=P)
    got = fetch_channel_messages(client, feed.chat_id_of(cid), cfg)
    return {m.msg_id for m in got}


def run_and_check(tmp_path, crawl_id="w1", chunk_channels=256, **cfg_kw):
    cfg, feed, sm, eng = mk_engine(tmp_path, crawl_id, chunk_channels,
                                   **cfg_kw)
    names = ["c%010d" % c for c in CIDS]
    discovered, posts = eng.process_channels(names, now=NOW)
    sm.close()
    files, link_names, keep, kept = expectation(feed, cfg)
    for k, cid in enumerate(CIDS):
        got = read_posts(tmp_path, crawl_id, cid)
        if not files[k]:
            assert got is None, f"channel {cid}: a file for no post"
            continue
        assert got == files[k], f"channel {cid} JSONL differs"
    assert set(discovered) == link_names
    n_lines = sum(f.count(b"\n") for f in files)
    assert posts == n_lines and eng.stats["posts"] == n_lines
    assert eng.stats["pages"] == len(CIDS)
    assert eng.last_deadends == set()
    return cfg, feed, eng, keep, kept


def test_window_only(tmp_path):
    feed = SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P))
    lo, hi = bounds(feed, 16, 48)
    cfg, feed, eng, keep, kept = run_and_check(
        tmp_path, date_between_min=ts(lo), date_between_max=ts(hi))
    # posts 16 .. 47, whatever their jitter
    assert kept.tolist() == [32] * 3
    assert keep[:, 16:48].all() and keep.sum() == 96
    assert eng.stats["posts"] == int(kept.sum())
    for cid in CIDS:
        got = msg_ids_of(read_posts(tmp_path, "w1", cid))
        assert got == cpu_fetch_ids(feed, cfg, cid)
        assert got == {(p + 1) << 20 for p in range(16, 48)}


def test_max_posts_alone_keeps_the_newest(tmp_path):
    cfg, feed, eng, keep, kept = run_and_check(tmp_path, max_posts=10)
    assert kept.tolist() == [10] * 3 and keep[:, P - 10:].all()
    for cid in CIDS:
        assert (msg_ids_of(read_posts(tmp_path, "w1", cid))
                == cpu_fetch_ids(feed, cfg, cid))


@pytest.mark.parametrize("max_posts,n", [(3, 3), (10, 6)])
def test_max_posts_with_min_post_date(tmp_path, max_posts, n):
    feed = SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P))
    lo, _ = bounds(feed, P - 6, P)
    cfg, feed, eng, keep, kept = run_and_check(
        tmp_path, max_posts=max_posts, min_post_date=ts(lo))
    assert kept.tolist() == [n] * 3
    for cid in CIDS:
        assert (msg_ids_of(read_posts(tmp_path, "w1", cid))
                == cpu_fetch_ids(feed, cfg, cid))


def test_window_with_sample_size(tmp_path):
    feed = SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P))
    lo, hi = bounds(feed, 10, 50)
    kw = dict(date_between_min=ts(lo), date_between_max=ts(hi),
              sample_size=7, sample_seed=5)
    cfg, feed, eng, keep, kept = run_and_check(tmp_path / "a", "s1", 1, **kw)
    assert kept.tolist() == [7] * 3
    assert not keep[:, :10].any() and not keep[:, 50:].any()
    # the channels do not all draw the same positions
    assert len({tuple(row) for row in keep.tolist()}) > 1
    run_and_check(tmp_path / "b", "s1", 256, **kw)
    for cid in CIDS:
        one = read_posts(tmp_path / "a", "s1", cid)
        assert one.count(b"\n") == 7
        assert one == read_posts(tmp_path / "b", "s1", cid)
    # another seed, another sample
    _, _, _, keep2, _ = run_and_check(tmp_path / "c", "s1", 256,
                                      **dict(kw, sample_seed=6))
    assert (keep2 != keep).any()


@pytest.mark.parametrize("chunk_channels", [1, 256])
def test_empty_window_for_one_channel(tmp_path, chunk_channels):
    feed = SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P))
    b, _lines, _links = golden(feed, CIDS)
    dates = b.meta["date"].numpy().reshape(3, P)
    # one second that holds a post of channels 3 and 17, none of 9
    second = [int(d) for d in dates[0] if d in dates[2] and d not in dates[1]]
    if second:
        lo = hi = second[0]
        want = [1, 0, 1]
    else:
        lo = hi = next(int(d) for d in dates[0] if d not in dates[1])
        want = [1, 0, int(lo in dates[2])]
    cfg, feed, eng, keep, kept = run_and_check(
        tmp_path, "w1", chunk_channels, date_between_min=ts(lo),
        date_between_max=ts(hi))
    assert kept.tolist() == want
    assert read_posts(tmp_path, "w1", 9) is None
    assert read_posts(tmp_path, "w1", 3).count(b"\n") == 1
    assert "c%010d" % 9 not in eng.last_deadends
    assert eng.stats["deadends"] == 0


@pytest.mark.parametrize("with_min_post_date", [False, True])
def test_without_a_window_the_kernel_is_never_launched(
        tmp_path, monkeypatch, with_min_post_date):
    from crawler_amd.ops import gpu

    feed = SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P))
    kw = {}
    if with_min_post_date:
        kw["min_post_date"] = ts(bounds(feed, 32, P)[0])
    real, launched = gpu._call, []

    def spy(name, *args, **kwargs):
        launched.append(name)
        return real(name, *args, **kwargs)

    monkeypatch.setattr(gpu, "_call", spy)
    cfg, feed, sm, eng = mk_engine(tmp_path, "g1",
                                   sampling_method="snowball", max_depth=1,
                                   **kw)
    assert gpu.window_params(cfg) is None
    names = ["c%010d" % c for c in CIDS]
    discovered, posts = eng.process_channels(names, now=NOW)
    sm.close()
    assert "crawl_measure_extract" in launched
    assert "crawl_fetch_window" not in launched
    _b, lines, links = golden(feed, CIDS, cfg.min_post_date)
    for k, cid in enumerate(CIDS):
        assert read_posts(tmp_path, "g1", cid) == b"".join(
            lines[k * P:(k + 1) * P]), f"channel {cid} JSONL differs"
    assert set(discovered) == {n for row in links for (n, _s) in row}
    assert posts == sum(1 for l in lines if l)
    assert posts == (3 * 32 if with_min_post_date else 3 * P)


def test_cli_gpu_date_between_sample_size_end_to_end(tmp_path):
    from crawler_amd.cli import main

    base = FeedConfig().base_date
    day = dt.datetime.fromtimestamp(base, UTC).replace(
        hour=0, minute=0, second=0, microsecond=0)
    nxt = day + dt.timedelta(days=1)
    # some of the 256 posts fall on the next day
    assert base + 255 * FeedConfig().date_step > nxt.timestamp()
    rc = main([
        "--mode", "standalone", "--gpu", "--sampling", "channel",
        "--urls", "c0000000001,c0000000002,c0000000007",
        "--storage-root", str(tmp_path), "--crawl-id", "gwin1",
        "--synthetic-universe", "300", "--synthetic-posts", "256",
        "--date-between", "%s,%s" % (day.strftime("%Y-%m-%d"),
                                     nxt.strftime("%Y-%m-%d")),
        "--sample-size", "5", "--sample-seed", "9",
        "--min-users", "1", "--skip-media",
    ])
    assert rc == 0
    prog = json.loads((tmp_path / "gwin1" / "progress.json").read_text())
    assert prog["status"] == "completed"
    jsonls = list((tmp_path / "gwin1").rglob("posts.jsonl"))
    assert len(jsonls) == 3
    for path in jsonls:
        lines = path.read_bytes().splitlines()
        assert 1 <= len(lines) <= 5
        for line in lines:
            at = dt.datetime.strptime(json.loads(line)["published_at"],
                                      "%Y-%m-%dT%H:%M:%SZ").replace(tzinfo=UTC)
            assert day <= at <= nxt
