"""replay_random_accounting vs the real SyntheticYouTubeClient, and the
YouTube plugin's --gpu dispatch (CPU-only: nothing here touches a GPU)."""
import random
import types

import pytest

from crawler_amd.config import CrawlerConfig
from crawler_amd.youtube.client import QuotaExceeded, SyntheticYouTubeClient
from crawler_amd.youtube.gpu_runner import replay_random_accounting
from crawler_amd.youtube.synth import SyntheticYouTubeIndex

MIN_CH = 10
BIG = 10 ** 12


def search_rows(index, rng, n_searches, min_channel_videos=MIN_CH):
    """Per-search (invalid, candidates, new_channels, verified) rows and
    the verified ids, from the index's own primitives."""
    seen, chan_seen = set(), set()
    rows, verified_ids = [], []
    for _ in range(n_searches):
        prefix = SyntheticYouTubeClient.generate_random_prefix(rng)
        inv = cand = newch = ver = 0
        for vid in index.search_prefix(prefix):
            if not SyntheticYouTubeClient.is_valid_sample(vid, prefix):
                inv += 1
                continue
            if vid in seen:
                continue
            seen.add(vid)
            cand += 1
            v = index.video(vid)
            if v.channel_id not in chan_seen:
                chan_seen.add(v.channel_id)
                newch += 1
            n = index.channel_index_of(v.channel_id)
            if index.channel(n).video_count > min_channel_videos:
                ver += 1
                verified_ids.append(vid)
        rows.append((inv, cand, newch, ver))
    return rows, verified_ids


def run_client(seed, universe, limit, max_searches, quota):
    client = SyntheticYouTubeClient(
        SyntheticYouTubeIndex(seed=seed, universe_channels=universe),
        daily_quota=quota, min_channel_videos=MIN_CH,
        rng=random.Random(11))
    vids = client.get_random_videos(limit, max_searches=max_searches)
    return client, [v.id for v in vids]


def rows_for(seed, universe, max_searches, limit, quota=BIG):
    # enough rows for the run: the loop cannot outlast max_searches or
    # the searches the quota pays for; test_replay_matches_client
    # asserts the replay stopped before the rows ran out
    n = min(max_searches, 2 * limit + 100, quota // 100 + 1)
    return search_rows(
        SyntheticYouTubeIndex(seed=seed, universe_channels=universe),
        random.Random(11), n)


CASES = [
    (5, 3000, 120, 10 ** 6, BIG),
    (5, 3000, 300, 50, BIG),        # the max_searches bound
    (5, 3000, 500, 10 ** 6, 10000),  # the quota break at a search
    (9, 100, 50, 10 ** 6, BIG),
    (9, 100, 77, 10 ** 6, BIG),
    (9, 100, 100, 10 ** 6, BIG),
]


@pytest.mark.parametrize("seed,universe,limit,max_searches,quota", CASES)
def test_replay_matches_client(seed, universe, limit, max_searches, quota):
    client, ids = run_client(seed, universe, limit, max_searches, quota)
    rows, verified = rows_for(seed, universe, max_searches, limit, quota)
    n, cut, stats, used = replay_random_accounting(
        rows, limit, max_searches, quota)
    assert cut < len(rows) or cut == max_searches
    assert n == len(ids)
    assert verified[:n] == ids
    assert stats == client.stats
    assert used == client.quota_used
    assert cut == client.stats["searches"]


def test_replay_known_ends():
    """The issue's two recorded CPU end states."""
    _, ids = run_client(5, 3000, 300, 50, BIG)
    assert len(ids) == 84
    _, ids = run_client(5, 3000, 500, 10 ** 6, 10000)
    assert len(ids) == 157


def test_replay_raises_where_a_list_unit_does_not_fit():
    """A quota at which a Videos.List / channel lookup, not a search, is
    the unit that does not fit: both sides raise."""
    seed, universe, limit = 5, 3000, 120
    client, _ = run_client(seed, universe, limit, 10 ** 6, BIG)
    rows, _ = rows_for(seed, universe, 10 ** 6, limit)
    total = client.quota_used
    hit = 0
    # the last unit spent is the final Videos.List; walk a few quotas
    # below the total so list and channel-lookup units are both covered
    for quota in range(total - 1, total - 8, -1):
        try:
            run_client(seed, universe, limit, 10 ** 6, quota)
            cpu_raised = False
        except QuotaExceeded:
            cpu_raised = True
        try:
            replay_random_accounting(rows, limit, 10 ** 6, quota)
            gpu_raised = False
        except QuotaExceeded:
            gpu_raised = True
        assert cpu_raised == gpu_raised, quota
        hit += cpu_raised
    assert hit >= 1


def test_replay_zero_limit_and_no_rows():
    assert replay_random_accounting([], 0, 10, 100)[:2] == (0, 0)
    n, cut, stats, used = replay_random_accounting([], 10, 10, 100)
    assert (n, cut, used) == (0, 0, 0) and stats["searches"] == 0


# ---------- plugin dispatch ----------

def _ctx(tmp_path, sampling, gpu, urls):
    from crawler_amd.registry import CrawlContext

    cfg = CrawlerConfig(storage_root=str(tmp_path), crawl_id="c",
                        platform="youtube", sampling_method=sampling,
                        max_posts=5, synthetic_seed=5)
    return CrawlContext(cfg=cfg, args=types.SimpleNamespace(gpu=gpu),
                        urls=urls, feed=None)


@pytest.fixture
def calls(monkeypatch):
    import crawler_amd.youtube.gpu_runner as gr
    import crawler_amd.youtube.runner as cr

    seen = {"gpu": 0, "cpu": 0}

    def fake_gpu(cfg, urls, **kw):
        seen["gpu"] += 1
        return {"videos": 0}

    def fake_cpu(cfg, urls, **kw):
        seen["cpu"] += 1
        return {"videos": 0}

    monkeypatch.setattr(gr, "run_youtube_gpu", fake_gpu)
    monkeypatch.setattr(cr, "run_youtube", fake_cpu)
    return seen


@pytest.mark.parametrize("sampling,urls", [("random", []),
                                           ("channel", ["3"])])
def test_plugin_gpu_dispatch(tmp_path, calls, capsys, sampling, urls):
    from crawler_amd.platforms.youtube import YouTubeCrawler

    YouTubeCrawler().run(_ctx(tmp_path, sampling, True, urls))
    assert calls == {"gpu": 1, "cpu": 0}
    assert "youtube gpu crawl complete" in capsys.readouterr().err


def test_plugin_without_gpu_runs_cpu(tmp_path, calls):
    from crawler_amd.platforms.youtube import YouTubeCrawler

    YouTubeCrawler().run(_ctx(tmp_path, "random", False, []))
    assert calls == {"gpu": 0, "cpu": 1}


def test_plugin_gpu_snowball_runs_cpu_with_notice(tmp_path, calls, capsys):
    from crawler_amd.platforms.youtube import YouTubeCrawler

    YouTubeCrawler().run(_ctx(tmp_path, "snowball", True, ["3"]))
    assert calls == {"gpu": 0, "cpu": 1}
    err = capsys.readouterr().err
    assert "GPU mode covers random and channel sampling" in err


def test_cli_flags_reach_config():
    from crawler_amd.cli import parse_config

    cfg = parse_config(["--platform", "youtube", "--yt-max-searches", "7",
                        "--yt-daily-quota", "12345"])
    assert (cfg.yt_max_searches, cfg.yt_daily_quota) == (7, 12345)
    cfg = parse_config(["--platform", "youtube"])
    assert (cfg.yt_max_searches, cfg.yt_daily_quota) == (200, 10000)
