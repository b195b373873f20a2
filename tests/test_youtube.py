"""YouTube subsystem tests (reference crawler/youtube/*_test.go coverage:
sampling dispatch, prefix validity rule, channel gate, quota economics,
duration parsing, video->Post conversion)."""
import json
import random

import pytest

from crawler_amd.config import CrawlerConfig
from crawler_amd.youtube import (
    QuotaExceeded,
    SyntheticYouTubeClient,
    SyntheticYouTubeIndex,
    convert_video_to_post,
    parse_iso8601_duration,
)
from crawler_amd.youtube.convert import extract_urls
from crawler_amd.youtube.runner import run_youtube


@pytest.fixture
def client():
    return SyntheticYouTubeClient(
        SyntheticYouTubeIndex(seed=5, universe_channels=500),
        rng=random.Random(1),
    )


# ---------- validity rule (youtube_client.go:1266-1281) ----------

@pytest.mark.parametrize("vid,prefix,ok", [
    ("abcde-12345", "abcde", True),
    ("abcde-1234", "abcde", False),     # len != 11
    ("abcdef12345", "abcde", False),    # no dash at 5
    ("xbcde-12345", "abcde", False),    # wrong prefix
])
def test_prefix_validity_rule(vid, prefix, ok):
    assert SyntheticYouTubeClient.is_valid_sample(vid, prefix) == ok


def test_random_prefix_shape():
    rng = random.Random(3)
    p = SyntheticYouTubeClient.generate_random_prefix(rng)
    assert len(p) == 5 and p.isalpha() and p.islower()


# ---------- duration parsing ----------

@pytest.mark.parametrize("s,secs", [
    ("PT5M30S", 330),
    ("PT1H2M3S", 3723),
    ("P1DT1S", 86401),
    ("PT45S", 45),
])
def test_iso8601_duration(s, secs):
    assert parse_iso8601_duration(s) == secs


def test_url_extraction_trims_punctuation():
    urls = extract_urls("see https://a.example/x, and (https://b.example/y).")
    assert urls == ["https://a.example/x", "https://b.example/y"]


@pytest.mark.parametrize("text,urls", [
    # a URL ends at the reference's byte-level \s = [\t\n\f\r ]
    # (youtube_crawler.go:61) or at this project's < > "
    ("http://a\tb", ["http://a"]),
    ("http://a\nb", ["http://a"]),
    ("http://a\x0cb", ["http://a"]),
    ("http://a\rb", ["http://a"]),
    ("http://a b", ["http://a"]),
    ("http://a<b", ["http://a"]),
    ("http://a>b", ["http://a"]),
    ('http://a"b', ["http://a"]),
    # everything else continues it: \v, other controls, DEL, non-ASCII
    # space and line separators (Python's Unicode \s would stop here)
    ("http://a\x0bb c", ["http://a\x0bb"]),
    ("http://a\x01b c", ["http://a\x01b"]),
    ("http://a\x1cb\x1fc d", ["http://a\x1cb\x1fc"]),
    ("http://a\x7fb c", ["http://a\x7fb"]),
    ("http://a\u00a0b c", ["http://a\u00a0b"]),
    ("http://a\u0085b c", ["http://a\u0085b"]),
    ("http://a\u2028b c", ["http://a\u2028b"]),
    ("http://a\u3000b c", ["http://a\u3000b"]),
    # a bare scheme is no URL; "http://." is (the dot is then trimmed)
    ("see http:// x", []),
    ("http://", []),
    ("http://<b", []),
    ("https://", []),
    ("http://.", ["http://"]),
    ("HTTP://a", []),
    ("hthttp://a httphttp://b", ["http://a", "http://b"]),
])
def test_url_extraction_stop_set(text, urls):
    assert extract_urls(text) == urls


def test_url_extraction_keeps_every_distinct_url_in_order():
    text = " ".join("https://e.example/%d," % (j % 10) for j in range(25))
    assert extract_urls(text) == ["https://e.example/%d" % j
                                  for j in range(10)]


# ---------- quota ----------

def test_quota_accounting(client):
    q0 = client.quota_used
    client.search("abcde")
    assert client.quota_used == q0 + 100
    client.list_videos(["abcde-12345"])
    assert client.quota_used == q0 + 101


def test_quota_exceeded_stops_sampling():
    c = SyntheticYouTubeClient(
        SyntheticYouTubeIndex(seed=5, universe_channels=100),
        daily_quota=150, rng=random.Random(1),
    )
    with pytest.raises(QuotaExceeded):
        c.search("aaaaa")
        c.search("bbbbb")


# ---------- random sampling ----------

def test_random_sampling_respects_gate_and_rule(client):
    videos = client.get_random_videos(limit=20, max_searches=40)
    assert videos
    for v in videos:
        assert len(v.id) == 11 and v.id[5] == "-"
        ch = client.get_channel_info(v.channel_id)
        assert ch.video_count > client.min_channel_videos
    assert client.stats["invalid_ids"] > 0  # noise ids got filtered
    assert client.stats["gate_rejected"] >= 0


# ---------- snowball ----------

def test_snowball_discovers_channels(client):
    seed = client.index.channel_id_of(7)
    client.index.channel(7)  # register in reverse map
    videos = client.get_snowball_videos([seed], limit=30, max_depth=2)
    assert videos
    chans = {v.channel_id for v in videos}
    assert len(chans) >= 1


# ---------- conversion ----------

def test_convert_video_to_post_fields(client):
    vid = client.index.video("abcde-12345")
    ch = client.get_channel_info(vid.channel_id)
    post = convert_video_to_post(vid, ch, crawl_label="yt-test")
    obj = json.loads(post.to_json())
    assert obj["platform_name"] == "youtube"
    assert obj["post_uid"] == "abcde-12345"
    assert obj["post_link"] == "https://www.youtube.com/watch?v=abcde-12345"
    assert obj["post_type"] == ["video"]
    assert obj["crawl_label"] == "yt-test"
    assert obj["engagement"] == (
        vid.like_count + vid.comment_count + vid.view_count // 100
    )
    assert obj["performance_scores"]["likes"] == vid.like_count
    assert obj["has_embed_media"] is True
    assert obj["post_title"] == vid.title
    assert obj["media_data"]["document_name"].endswith(".mp4")
    if vid.duration == "P0D":
        assert obj["video_length"] is None
    assert obj["outlinks"]  # description contains URLs


def test_p0d_duration_null(client):
    vid = client.index.video("abcde-12345")
    vid.duration = "P0D"
    post = convert_video_to_post(vid, None)
    assert post.video_length is None


# ---------- runner ----------

def test_run_youtube_random_mode(tmp_path):
    cfg = CrawlerConfig(crawl_id="yt1", storage_root=str(tmp_path),
                        platform="youtube", sampling_method="random",
                        max_posts=10)
    stats = run_youtube(cfg, [])
    assert stats["posts"] >= 1
    assert stats["quota_used"] > 0
    # posts landed in per-channel JSONL files
    crawl_dir = tmp_path / "yt1"
    jsonls = list(crawl_dir.rglob("posts.jsonl"))
    assert jsonls
    obj = json.loads(jsonls[0].read_bytes().splitlines()[0])
    assert obj["platform_name"] == "youtube"


def test_run_youtube_channel_mode(tmp_path):
    cfg = CrawlerConfig(crawl_id="yt2", storage_root=str(tmp_path),
                        platform="youtube", sampling_method="channel",
                        max_posts=20)
    stats = run_youtube(cfg, ["3"])
    assert stats["videos"] >= 1


def test_client_pool_rotation():
    """ytWorker rotation (dapr/standalone.go:1245-1272): retire ~50+-10."""
    import random as _r

    from crawler_amd.youtube.client import YouTubeClientPool

    made = []

    def mk():
        c = SyntheticYouTubeClient(
            SyntheticYouTubeIndex(seed=1, universe_channels=10)
        )
        made.append(c)
        return c

    pool = YouTubeClientPool(mk, retire_at=50, retire_jitter=10,
                             rng=_r.Random(5))
    for _ in range(200):
        pool.get()
    assert pool.retired >= 2
    assert 3 <= len(made) <= 6  # ~200/50 rotations


def test_build_corpus_deterministic_bytes():
    """Same seed -> byte-identical encoded corpus (the bench relies on
    deterministic regeneration across processes/boxes)."""
    import datetime as dt

    from crawler_amd.youtube.batch import build_corpus, encode_yt_batch
    from crawler_amd.youtube.synth import SyntheticYouTubeIndex

    NOW = dt.datetime(2026, 1, 1, tzinfo=dt.timezone.utc)
    a = build_corpus(SyntheticYouTubeIndex(seed=99), 50,
                     crawl_label="det")
    b = build_corpus(SyntheticYouTubeIndex(seed=99), 50,
                     crawl_label="det")
    la = encode_yt_batch(a, now=NOW)
    lb = encode_yt_batch(b, now=NOW)
    assert b"".join(la) == b"".join(lb)
    c = build_corpus(SyntheticYouTubeIndex(seed=100), 50,
                     crawl_label="det")
    lc = encode_yt_batch(c, now=NOW)
    assert b"".join(la) != b"".join(lc)


def test_build_corpus_fast_matches_slow():
    """Vectorized corpus builder is byte-identical to the per-video
    path through the whole encode pipeline (bench setup went from
    ~140 us/video to ~3 us/video)."""
    import datetime as dt

    from crawler_amd.youtube.batch import (build_corpus,
                                           build_corpus_fast,
                                           encode_yt_batch)
    from crawler_amd.youtube.synth import SyntheticYouTubeIndex

    now = dt.datetime(2026, 1, 1, tzinfo=dt.timezone.utc)
    slow = build_corpus(SyntheticYouTubeIndex(seed=99,
                                              universe_channels=50_000),
                        1200, crawl_label="x")
    fast = build_corpus_fast(
        SyntheticYouTubeIndex(seed=99, universe_channels=50_000),
        1200, crawl_label="x")
    assert encode_yt_batch(slow, now=now) == encode_yt_batch(fast,
                                                             now=now)
    assert fast.n_channels == slow.n_channels


def test_youtube_runner_applies_date_window(tmp_path):
    """run_youtube filters fetched videos through the
    CalculateDateFilters window (dapr/standalone.go:1119-1147 passes
    the range into the crawl job)."""
    import datetime as dt

    from crawler_amd.config import CrawlerConfig
    from crawler_amd.engine import LocalStateManager
    from crawler_amd.youtube.runner import run_youtube

    UTC = dt.timezone.utc
    base_cfg = dict(crawl_id="ytd", storage_root=str(tmp_path),
                    platform="youtube", sampling_method="channel",
                    min_users=1, max_posts=50)
    cfg_all = CrawlerConfig(**base_cfg)
    sm1 = LocalStateManager(cfg_all)
    stats_all = run_youtube(cfg_all, ["3"], sm=sm1)

    # a window far in the past excludes everything
    cfg_none = CrawlerConfig(
        **{**base_cfg, "crawl_id": "ytd2"},
        date_between_min=dt.datetime(1990, 1, 1, tzinfo=UTC),
        date_between_max=dt.datetime(1991, 1, 1, tzinfo=UTC))
    sm2 = LocalStateManager(cfg_none)
    stats_none = run_youtube(cfg_none, ["3"], sm=sm2)
    assert stats_all["posts"] > 0
    assert stats_none["posts"] == 0
    # like the reference (the range rides in the crawl job), the video
    # count reflects the filtered window
    assert stats_none["videos"] == 0


def test_build_corpus_fast_matches_slow_from_i0():
    """The first-index parameter of both host builders: rows i0..i0+n
    are the same videos, also across the 26**5 prefix wrap."""
    import datetime as dt

    from crawler_amd.youtube.batch import (build_corpus,
                                           build_corpus_fast,
                                           encode_yt_batch)
    from crawler_amd.youtube.synth import SyntheticYouTubeIndex

    now = dt.datetime(2026, 1, 1, tzinfo=dt.timezone.utc)
    mk = lambda: SyntheticYouTubeIndex(seed=17, universe_channels=63)
    whole = encode_yt_batch(build_corpus(mk(), 96), now=now)
    assert encode_yt_batch(build_corpus(mk(), 64, i0=32), now=now) \
        == whole[32:]
    assert encode_yt_batch(build_corpus_fast(mk(), 64, i0=32), now=now) \
        == whole[32:]
    wrap = 26 ** 5
    slow = build_corpus(mk(), 64, i0=wrap - 32)
    fast = build_corpus_fast(mk(), 64, i0=wrap - 32)
    lines = encode_yt_batch(slow, now=now)
    assert encode_yt_batch(fast, now=now) == lines
    assert fast.n_channels == slow.n_channels
    assert b'"post_uid":"zzzzz-' in lines[31]
    assert b'"post_uid":"aaaaa-' in lines[32]
