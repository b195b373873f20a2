"""SnowballReplay vs the real SyntheticYouTubeClient.get_snowball_videos,
and the YouTube plugin's --yt-gpu-snowball dispatch (CPU-only: nothing
here touches a GPU)."""
import re
import types

import pytest

from crawler_amd.config import CrawlerConfig
from crawler_amd.youtube.client import QuotaExceeded, SyntheticYouTubeClient
from crawler_amd.youtube.gpu_runner import SnowballReplay
from crawler_amd.youtube.synth import SyntheticYouTubeIndex

BIG = 10 ** 12
SEEDS = [82, 99, 33, 99]   # 82 has no uploads; 99 is repeated
DEPTH = 1
CID_RE = re.compile(r"UC[0-9A-Za-z_-]{22}")


def _index():
    return SyntheticYouTubeIndex(seed=5, universe_channels=3000)


def visit_order(index, seeds, max_depth):
    """The channels an unlimited crawl visits, in order, with their upload
    ids: a plain BFS over the index's own primitives (no client, no
    quota, no limit)."""
    frontier = [index.channel_id_of(n) for n in seeds]
    visited, out, depth = set(), [], 0
    while frontier and depth <= max_depth:
        nxt = []
        for cid in frontier:
            if cid in visited:
                continue
            visited.add(cid)
            ids = index.channel_uploads(cid)
            out.append(ids)
            for vid in ids:
                nxt.extend(CID_RE.findall(index.video(vid).description))
        frontier = nxt
        depth += 1
    return out


@pytest.fixture(scope="module")
def visits():
    return visit_order(_index(), SEEDS, DEPTH)


def run_client(limit, quota):
    index = _index()
    client = SyntheticYouTubeClient(index, daily_quota=quota)
    seeds = [index.channel_id_of(n) for n in SEEDS]
    try:
        vids = client.get_snowball_videos(seeds, limit, max_depth=DEPTH)
        return client, [v.id for v in vids], False
    except QuotaExceeded:
        return client, None, True


def run_replay(visits, limit, quota):
    rp = SnowballReplay(limit, quota)
    counts = [len(ids) for ids in visits]
    try:
        used = rp.feed(counts)
        return rp, used, False
    except QuotaExceeded:
        return rp, None, True


def _ends(visits):
    ends, total = [], 0
    for ids in visits:
        if ids:
            total += len(ids)
            ends.append(total)
    return ends


def test_visit_order_has_the_cases(visits):
    counts = [len(ids) for ids in visits]
    assert counts[0] == 0                      # channel 82
    assert len(visits) > 3 + 5                 # depth 1 was reached
    assert sum(counts) == 545                  # the recorded CPU figure
    assert 0 in counts[3:]                     # a discovered empty channel


def _limits(visits):
    ends = _ends(visits)
    return [1, ends[0] - 4, ends[0], ends[0] + 1, ends[2], ends[2] + 1,
            ends[5] - 1, ends[5], ends[-1] - 1, ends[-1], ends[-1] + 10]


def test_replay_matches_client_over_limits(visits):
    flat = [vid for ids in visits for vid in ids]
    limits = _limits(visits)
    ends = _ends(visits)
    assert any(lim in ends for lim in limits)          # cut at an end
    assert any(lim not in ends and lim < ends[-1] for lim in limits)
    for limit in limits:
        client, ids, raised = run_client(limit, BIG)
        rp, used, r_raised = run_replay(visits, limit, BIG)
        assert not raised and not r_raised
        assert rp.videos == len(ids), limit
        assert flat[:rp.videos] == ids, limit
        assert rp.quota_used == client.quota_used, limit
        assert rp.stats == client.stats, limit
        assert rp.done == (len(ids) >= limit), limit
        if rp.done:
            # the cut channel is the last one consumed
            assert sum(len(v) for v in visits[:used]) >= limit
            assert sum(len(v) for v in visits[:used - 1]) < limit
        else:
            assert used == len(visits)


def test_replay_matches_client_under_tight_quotas(visits):
    units = sum(1 for ids in visits if ids)    # one Videos.List each
    hit = 0
    for quota in (0, 1, 2, 9, units - 1, units, units + 1):
        for limit in (137, BIG):
            client, ids, raised = run_client(limit, quota)
            rp, _, r_raised = run_replay(visits, limit, quota)
            assert raised == r_raised, (quota, limit)
            # where it raises: the same units spent, the same batches
            assert rp.quota_used == client.quota_used, (quota, limit)
            assert rp.stats == client.stats, (quota, limit)
            if not raised:
                assert rp.videos == len(ids)
            hit += raised
    assert hit >= 4
    # the issue's recorded case: limit 137 over seeds 99, 33 costs 9 units
    client, ids, _ = run_client(137, BIG)
    assert (len(ids), client.quota_used) == (137, 9)


def test_replay_feeds_layer_by_layer(visits):
    """Feeding in pieces (the runner feeds one BFS layer at a time) is
    the same as feeding at once."""
    counts = [len(ids) for ids in visits]
    whole = SnowballReplay(300, BIG)
    whole.feed(counts)
    parts = SnowballReplay(300, BIG)
    used = parts.feed(counts[:4])
    assert used == 4 and not parts.done
    used = parts.feed(counts[4:])
    assert parts.done and used < len(counts) - 4
    assert parts.feed(counts) == 0             # done: consumes nothing
    assert (parts.videos, parts.quota_used, parts.stats) == (
        whole.videos, whole.quota_used, whole.stats)
    assert parts.videos == 300


def test_replay_zero_limit():
    rp = SnowballReplay(0, 100)
    assert rp.done and rp.feed([5, 5]) == 0 and rp.quota_used == 0


# ---------- plugin dispatch ----------

def _ctx(tmp_path, args):
    from crawler_amd.registry import CrawlContext

    cfg = CrawlerConfig(storage_root=str(tmp_path), crawl_id="c",
                        platform="youtube", sampling_method="snowball",
                        max_posts=5, synthetic_seed=5)
    return CrawlContext(cfg=cfg, args=types.SimpleNamespace(**args),
                        urls=["3"], feed=None)


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


def test_plugin_snowball_flag_dispatches_to_gpu(tmp_path, calls, capsys):
    from crawler_amd.platforms.youtube import YouTubeCrawler

    YouTubeCrawler().run(_ctx(tmp_path, dict(gpu=True,
                                             yt_gpu_snowball=True)))
    assert calls == {"gpu": 1, "cpu": 0}
    err = capsys.readouterr().err
    assert "youtube gpu crawl complete" in err
    assert "running snowball on the CPU" not in err


@pytest.mark.parametrize("args", [dict(gpu=True, yt_gpu_snowball=False),
                                  dict(gpu=True)])
def test_plugin_snowball_without_flag_runs_cpu(tmp_path, calls, capsys,
                                               args):
    from crawler_amd.platforms.youtube import YouTubeCrawler

    YouTubeCrawler().run(_ctx(tmp_path, args))
    assert calls == {"gpu": 0, "cpu": 1}
    err = capsys.readouterr().err
    assert "GPU mode covers random and channel sampling" in err
    assert "--yt-gpu-snowball" in err


def test_plugin_flag_without_gpu_runs_cpu(tmp_path, calls, capsys):
    from crawler_amd.platforms.youtube import YouTubeCrawler

    YouTubeCrawler().run(_ctx(tmp_path, dict(gpu=False,
                                             yt_gpu_snowball=True)))
    assert calls == {"gpu": 0, "cpu": 1}
    assert "GPU mode covers" not in capsys.readouterr().err


def test_cli_flag_reaches_args():
    from crawler_amd.cli import build_parser, parse_config

    base = ["--platform", "youtube", "--sampling", "snowball", "--gpu"]
    assert build_parser().parse_args(base).yt_gpu_snowball is False
    assert build_parser().parse_args(
        base + ["--yt-gpu-snowball"]).yt_gpu_snowball is True
    cfg = parse_config(base + ["--yt-gpu-snowball"])
    assert cfg._cli.yt_gpu_snowball is True
