"""run_youtube_gpu snowball sampling end to end vs the CPU crawl:
byte-identical per-channel posts.jsonl files, identical file sets and
stats. A CPU reference is computed once per parameter set and shared."""
import datetime as dt
import os

import pytest

from crawler_amd.config import CrawlerConfig, calculate_date_filters
from crawler_amd.engine.state import LocalStateManager
from crawler_amd.youtube.client import QuotaExceeded, SyntheticYouTubeClient
from crawler_amd.youtube.convert import convert_video_to_post
from crawler_amd.youtube.synth import SyntheticYouTubeIndex

pytestmark = pytest.mark.gpu

NOW = dt.datetime(2026, 3, 4, 5, 6, 7, 123456, tzinfo=dt.timezone.utc)
LABEL = "yt-gpu"
BIG = 10 ** 12
NO_LIMIT = 10 ** 9
SEEDS = ("82", "99", "33", "99")   # 82: no uploads; 99 twice


def _index(universe=3000):
    return SyntheticYouTubeIndex(seed=5, universe_channels=universe)


def _index_with_uc():
    idx = _index()
    idx.channel_id_of(21)   # registers the id in the reverse map
    return idx


def _cfg(root, max_posts, max_depth, **kw):
    return CrawlerConfig(storage_root=str(root), crawl_id="crawl",
                         platform="youtube", sampling_method="snowball",
                         max_posts=max_posts, max_depth=max_depth,
                         crawl_label=LABEL, min_channel_videos=10, **kw)


def _tree(root):
    out = {}
    base = os.path.join(str(root), "crawl")
    for d, _, files in os.walk(base):
        for f in files:
            if f == "posts.jsonl":
                p = os.path.join(d, f)
                with open(p, "rb") as fh:
                    out[os.path.relpath(p, base)] = fh.read()
    return out


def cpu_crawl(cfg, urls, daily_quota, index):
    """youtube/runner.run_youtube's snowball path with a fixed `now` (the
    runner itself stamps wall-clock time)."""
    client = SyntheticYouTubeClient(
        index, daily_quota=daily_quota,
        min_channel_videos=cfg.min_channel_videos)
    resolved = [s if s.startswith("UC") else index.channel_id_of(int(s))
                for s in urls]
    videos = client.get_snowball_videos(resolved, cfg.max_posts,
                                        max_depth=max(cfg.max_depth, 1))
    from_t, to_t = calculate_date_filters(cfg)
    if from_t is not None:
        videos = [v for v in videos if from_t <= v.published_at <= to_t]
    sm = LocalStateManager(cfg)
    for v in videos:
        post = convert_video_to_post(
            v, client.get_channel_info(v.channel_id), crawl_label=LABEL,
            now=NOW)
        sm.store_post(post.channel_id, post)
    sm.save_state()
    sm.close()
    return {"videos": len(videos), "posts": len(videos),
            "quota_used": client.quota_used, **client.stats}


_REFS = {}


@pytest.fixture(scope="module")
def cpu_ref(tmp_path_factory):
    """(stats, tree) of the CPU crawl, computed once per parameter set."""
    def get(urls, max_posts, max_depth, index_factory=_index, window=None):
        key = (tuple(urls), max_posts, max_depth, index_factory, window)
        if key not in _REFS:
            root = tmp_path_factory.mktemp("cpu")
            cfg = _cfg(root, max_posts, max_depth, **dict(window or ()))
            stats = cpu_crawl(cfg, list(urls), BIG, index_factory())
            _REFS[key] = (stats, _tree(root))
        return _REFS[key]
    return get


def _gpu(tmp_path, cpu_ref, urls, max_posts, max_depth,
         index_factory=_index, window=None, **gpu_kw):
    from crawler_amd.youtube.gpu_runner import run_youtube_gpu

    want, ct = cpu_ref(urls, max_posts, max_depth, index_factory, window)
    cfg = _cfg(tmp_path / "gpu", max_posts, max_depth,
               **dict(window or ()))
    got = run_youtube_gpu(cfg, list(urls), now=NOW, daily_quota=BIG,
                          index=index_factory(), **gpu_kw)
    gt = _tree(tmp_path / "gpu")
    assert sorted(gt) == sorted(ct)
    for path in ct:
        assert gt[path] == ct[path], path
    assert got == want
    return want, ct


def _sampling_units(want, tree):
    # after sampling every distinct video channel costs one lookup
    return want["quota_used"] - len(tree)


def test_depth2_no_limit(tmp_path, cpu_ref):
    timings = {}
    want, tree = _gpu(tmp_path, cpu_ref, SEEDS, NO_LIMIT, 2,
                      timings=timings)
    assert want["videos"] == 7058 and len(tree) > 1000
    assert timings["snowball_layers"] == 3
    assert want["video_batches"] == _sampling_units(want, tree)


def test_depth2_small_chunks_and_table_growth(tmp_path, cpu_ref):
    """Chunked description scans and first-claim growth inside the crawl
    change nothing."""
    timings = {}
    want, _ = _gpu(tmp_path, cpu_ref, SEEDS, NO_LIMIT, 2, timings=timings,
                   chunk_videos=100, claim_slots_log2=4)
    assert want["videos"] == 7058
    assert timings["claim_grown"] >= 1


def test_fanout_stays_inside_the_open_file_limit(tmp_path, cpu_ref):
    """2710 channel files under an open-file limit that one fan-out call
    with all of them would exceed (a 100k-channel crawl met the same wall
    at the usual limits)."""
    import resource

    cpu_ref(SEEDS, NO_LIMIT, 2)     # computed under the usual limit
    n_open = len(os.listdir("/proc/self/fd"))
    assert n_open < 1500            # else the limit below proves nothing
    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    low = 2 * n_open + 1200
    if soft != resource.RLIM_INFINITY:
        low = min(low, soft)
    resource.setrlimit(resource.RLIMIT_NOFILE, (low, hard))
    try:
        want, tree = _gpu(tmp_path, cpu_ref, SEEDS, NO_LIMIT, 2)
    finally:
        resource.setrlimit(resource.RLIMIT_NOFILE, (soft, hard))
    assert len(tree) == 2710 > n_open + 1200


def test_depth1_no_limit(tmp_path, cpu_ref):
    want, _ = _gpu(tmp_path, cpu_ref, SEEDS, NO_LIMIT, 1)
    assert want["videos"] == 545


def test_depth_below_one_counts_as_one(tmp_path, cpu_ref):
    """max_depth = max(cfg.max_depth, 1): the config default is -1."""
    want, _ = _gpu(tmp_path, cpu_ref, SEEDS, NO_LIMIT, -1)
    assert want["videos"] == 545


def test_limit_cuts_inside_a_channel(tmp_path, cpu_ref):
    want, tree = _gpu(tmp_path, cpu_ref, ("99", "33"), 137, 3)
    assert want["videos"] == 137
    assert _sampling_units(want, tree) == 9 == want["video_batches"]


def test_limit_cuts_inside_the_first_channel(tmp_path, cpu_ref):
    want, tree = _gpu(tmp_path, cpu_ref, ("99",), 25, 2)
    assert want["videos"] == 25
    assert _sampling_units(want, tree) == 1


def _small_index():
    return _index(300)


def test_frontier_dies_out(tmp_path, cpu_ref):
    want, tree = _gpu(tmp_path, cpu_ref, ("150",), NO_LIMIT, 12,
                      index_factory=_small_index)
    assert want["videos"] == 4530
    assert _sampling_units(want, tree) == 297


def test_frontier_dies_out_before_depth_6(tmp_path, cpu_ref):
    """Depth 6 crawls what depth 12 does (the client's own crawl says so
    below), so the depth-12 reference serves."""
    from crawler_amd.youtube.gpu_runner import run_youtube_gpu

    def crawl(depth):
        idx = _small_index()
        c = SyntheticYouTubeClient(idx, daily_quota=BIG)
        vids = c.get_snowball_videos([idx.channel_id_of(150)], NO_LIMIT,
                                     max_depth=depth)
        return [v.id for v in vids], c.quota_used

    assert crawl(6) == crawl(12)
    want, ct = cpu_ref(("150",), NO_LIMIT, 12, _small_index, None)
    cfg = _cfg(tmp_path / "gpu", NO_LIMIT, 6)
    got = run_youtube_gpu(cfg, ["150"], now=NOW, daily_quota=BIG,
                          index=_small_index())
    assert _tree(tmp_path / "gpu") == ct
    assert got == want


def test_daily_quota_raises_on_both_sides(tmp_path):
    from crawler_amd.youtube.gpu_runner import run_youtube_gpu

    ccfg = _cfg(tmp_path / "cpu", NO_LIMIT, 2)
    gcfg = _cfg(tmp_path / "gpu", NO_LIMIT, 2)
    with pytest.raises(QuotaExceeded):
        cpu_crawl(ccfg, ["99", "33"], 12, _index())
    with pytest.raises(QuotaExceeded):
        run_youtube_gpu(gcfg, ["99", "33"], now=NOW, daily_quota=12,
                        index=_index())
    assert _tree(tmp_path / "cpu") == {} == _tree(tmp_path / "gpu")


PARTIAL = (
    ("date_between_min", dt.datetime(2024, 1, 1, tzinfo=dt.timezone.utc)),
    ("date_between_max", dt.datetime(2024, 2, 1, 0, 0, 0, 500000,
                                     tzinfo=dt.timezone.utc)))


def test_partial_date_window(tmp_path, cpu_ref):
    """The conversion pool looks up only the channels of videos that
    survive the window, so the filter moves quota_used too."""
    want, _ = _gpu(tmp_path, cpu_ref, SEEDS, NO_LIMIT, 1, window=PARTIAL)
    plain, _ = cpu_ref(SEEDS, NO_LIMIT, 1)
    assert 0 < want["videos"] < 545
    assert want["video_batches"] == plain["video_batches"]
    assert want["quota_used"] < plain["quota_used"]


def test_uc_seed_registered_in_the_index(tmp_path, cpu_ref):
    urls = ("82", _index().channel_id_of(21), "33")
    want, _ = _gpu(tmp_path, cpu_ref, urls, NO_LIMIT, 1,
                   index_factory=_index_with_uc)
    assert want["videos"] > 11 + 10


def test_unknown_uc_seed_raises(tmp_path):
    from crawler_amd.youtube.gpu_runner import run_youtube_gpu

    cfg = _cfg(tmp_path, 20, 2)
    with pytest.raises(ValueError, match="UCnot-a-known-channel"):
        run_youtube_gpu(cfg, ["99", "UCnot-a-known-channel__"], now=NOW,
                        index=_index())
    assert _tree(tmp_path) == {}
