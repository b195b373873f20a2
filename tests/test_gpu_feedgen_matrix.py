"""Device feed generator (csrc/feedgen.hip, three kernels) vs the numpy
builder over the matrix of tests/_corpora.py feed_cases(): odd shapes, a
batch the capped fill grid has to stride over, channel ids out of order /
repeated / past the universe, every comment rate and cap, the universe and
seed extremes, and dates that wrap through int32. Every tensor of the
batch must be bit-identical. test_aux_corpora_preconditions checks on the
CPU that the matrix picks every template and reaches the comment, entity
and reaction paths."""
import numpy as np
import pytest
import torch

import _corpora as C
from crawler_amd.feed import FeedConfig, SyntheticFeed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_FEED_KERNELS = ("crawl_feed_meta", "crawl_feed_fill", "crawl_feed_comments")
_CASES = C.feed_cases()


def _build_both(cfg, ids, P):
    feed = SyntheticFeed(FeedConfig(**cfg))
    ids = np.array(ids, dtype=np.int64)
    cpu_b = feed.build_batch(ids, posts_per_channel=P)
    dev_b = feed.build_batch_device(ids, DEV, posts_per_channel=P)
    torch.cuda.synchronize()
    return feed, ids, cpu_b, dev_b


@pytest.mark.parametrize("k", range(len(_CASES)),
                         ids=[c[0] for c in _CASES])
def test_feed_matrix_bit_identical(k):
    _, cfg, ids, P = _CASES[k]
    _, _, cpu_b, dev_b = _build_both(cfg, ids, P)
    assert cpu_b.n == len(ids) * P
    C.assert_batches_equal(cpu_b, dev_b)


@pytest.mark.parametrize("K,P", C.FEED_FORCED)
def test_feed_one_block_strides_over_the_batch(K, P, monkeypatch):
    """All three kernels launched with one block: every message and
    comment past the first 4 waves / 256 threads comes from a later trip
    of the grid-stride loop."""
    feed, ids, cpu_b, dev_b = _build_both(C.FEED_FORCED_CFG,
                                          list(range(10, 10 + K)), P)
    C.assert_batches_equal(cpu_b, dev_b)
    seen = C.force_grid_one(monkeypatch, _FEED_KERNELS)
    one_b = feed.build_batch_device(ids, DEV, posts_per_channel=P)
    torch.cuda.synchronize()
    assert seen == list(_FEED_KERNELS)
    C.assert_batches_equal(cpu_b, one_b)
    C.assert_batches_equal(dev_b.to("cpu"), one_b)


def test_feed_many_entity_rows_per_message(monkeypatch):
    """Messages with 0, 1, 4 and 70 entity rows (feed_entity_templates):
    every row of a message lands in its own slot, at the default grid and
    with one block."""
    cfg, ids, P = C.FEED_ENTITY_CASE
    feed = SyntheticFeed(FeedConfig(**cfg), C.feed_entity_templates())
    ids = np.array(ids, dtype=np.int64)
    cpu_b = feed.build_batch(ids, posts_per_channel=P)
    dev_b = feed.build_batch_device(ids, DEV, posts_per_channel=P)
    torch.cuda.synchronize()
    C.assert_batches_equal(cpu_b, dev_b)
    C.force_grid_one(monkeypatch, _FEED_KERNELS)
    one_b = feed.build_batch_device(ids, DEV, posts_per_channel=P)
    torch.cuda.synchronize()
    C.assert_batches_equal(cpu_b, one_b)


def test_feed_without_channels_is_empty_and_launches_nothing(monkeypatch):
    feed = SyntheticFeed(FeedConfig(seed=77, universe=1000))
    ids = np.zeros(0, dtype=np.int64)
    cpu_b = feed.build_batch(ids, posts_per_channel=5)
    C.forbid_launches(monkeypatch)
    dev_b = feed.build_batch_device(ids, DEV, posts_per_channel=5)
    assert dev_b.n == 0 and dev_b.n_channels == 0
    assert dev_b.device.type == "cuda"
    C.assert_batches_equal(cpu_b, dev_b)
    dev_b = feed.build_batch_device([], DEV, posts_per_channel=5)
    C.assert_batches_equal(cpu_b, dev_b)


@pytest.mark.parametrize("mc", [0, -1])
def test_feed_device_needs_room_for_a_comment(mc, monkeypatch):
    C.forbid_launches(monkeypatch)
    feed = SyntheticFeed(FeedConfig(seed=1, universe=10, comment_rate=0.5,
                                    max_comments_per_post=mc))
    with pytest.raises(ValueError):
        feed.build_batch_device(np.arange(2), DEV, posts_per_channel=3)


def test_feed_device_rate_zero_ignores_the_comment_cap():
    for mc in (0, -1):
        cfg = dict(seed=1, universe=10, comment_rate=0.0,
                   max_comments_per_post=mc)
        _, _, cpu_b, dev_b = _build_both(cfg, [0, 1], 3)
        assert cpu_b.com_text_off.numel() == 0
        C.assert_batches_equal(cpu_b, dev_b)


@pytest.mark.parametrize("rate", [0.0005, 0.0015, 0.9999])
def test_feed_device_refuses_a_rate_off_the_per_mille_grid(rate,
                                                           monkeypatch):
    """The kernel takes the rate as whole per-mille; a rate between two
    steps must raise, never round."""
    C.forbid_launches(monkeypatch)
    feed = SyntheticFeed(FeedConfig(seed=1, universe=10, comment_rate=rate))
    with pytest.raises(ValueError):
        feed.build_batch_device(np.arange(2), DEV, posts_per_channel=3)
