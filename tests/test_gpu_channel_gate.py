"""The channel-gate and compact-rows kernels (csrc/channel_gate.hip)
against their oracle (ops/golden_gate.py), bit for bit: tile tails, more
channels than a block has waves, the grid stride, ties, the kept == 0
fallback, sampled keep masks, and outputs that start out poisoned."""
import functools
import types

import numpy as np
import pytest
import torch

from _corpora import forbid_launches, force_grid_one
from _gate_cases import HAND_CASES, HAND_DATE, HAND_K, HAND_MSG, HAND_P
from crawler_amd.ops import golden_gate as GG
from crawler_amd.ops import golden_window as GW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = [1, 4, 5, 9]
PS = [1, 63, 64, 65, 130]
LO, HI = 1000, 2000   # every date lies in [LO, HI]


def fake_batch(date, msg, K, P):
    """The fields the window, the gate and the compaction read."""
    chat = np.repeat(-(1001000000000 + 3 * np.arange(K, dtype=np.int64) + 1),
                     P)
    t = lambda a, dt_: torch.tensor(np.asarray(a), dtype=dt_, device=DEV)
    return types.SimpleNamespace(
        device=torch.device(DEV), n=K * P, n_channels=K,
        meta={"date": t(date, torch.int32)},
        chat_id=t(chat, torch.int64), msg_id=t(msg, torch.int64)), chat


@functools.lru_cache(maxsize=None)
def arrays(K, P):
    """(date, msg_id, {name: keep}) of a K x P batch: dates without any
    order, msg_ids shuffled within a channel (the greatest is rarely the
    last row), and keep masks."""
    rng = np.random.default_rng(77 * K + P)
    date = rng.integers(LO, HI + 1, K * P).astype(np.int32)
    msg = np.concatenate([(rng.permutation(P).astype(np.int64) + 1) << 20
                          for _ in range(K)])
    masks = {
        "all": np.ones(K * P, dtype=np.uint8),
        "none": np.zeros(K * P, dtype=np.uint8),
        "sample": (rng.random(K * P) < 0.25).astype(np.uint8),
        "nonbinary": ((rng.random(K * P) < 0.5)
                      * rng.integers(1, 256, K * P)).astype(np.uint8),
    }
    mixed = masks["sample"].copy()
    mixed.reshape(K, P)[::2] = 0      # every second channel fetched nothing
    masks["some-empty"] = mixed
    return date, msg, masks


def kept_of(keep, K, P):
    return (keep.reshape(K, P) != 0).sum(1).astype(np.int32)


def run_gate(batch, keep, kept, recency):
    from crawler_amd.ops import gpu

    keep_t = torch.tensor(keep, device=DEV)
    kept_t = torch.tensor(kept, device=DEV)
    k2, n2, active, latest = gpu.channel_gate(batch, keep_t, kept_t,
                                              recency, _poison=0xFF)
    assert k2 is keep_t and n2 is kept_t, "keep and kept are in place"
    assert active.dtype == torch.uint8 and latest.dtype == torch.int32
    return keep_t, kept_t, active, latest


def check_gate(date, msg, K, P, keep, recency, batch=None):
    from crawler_amd.ops import gpu

    batch = batch or fake_batch(date, msg, K, P)[0]
    kept = kept_of(keep, K, P)
    want = GG.channel_gate(date, msg, P, K, recency, keep, kept)
    keep_t, kept_t, active, latest = run_gate(batch, keep, kept, recency)
    for name, got, exp in zip(("keep", "kept", "active", "latest"),
                              (keep_t, kept_t, active, latest), want):
        got = got.cpu().numpy()
        assert got.dtype == exp.dtype and got.tolist() == exp.tolist(), (
            name, recency)
    rows, chan = gpu.compact_rows(batch, keep_t, kept_t, _poison=0xFF)
    assert rows.dtype == torch.int64 and chan.dtype == torch.int32
    want_rows, want_chan = GG.compact_rows(want[0], want[1], P, K)
    assert rows.cpu().numpy().tolist() == want_rows.tolist(), recency
    assert chan.cpu().numpy().tolist() == want_chan.tolist(), recency
    assert rows.cpu().numpy().tolist() == np.flatnonzero(want[0]).tolist()
    return want


def recencies(date, msg, K, P, keep):
    """Below every date, above every date, between the channels' newest
    dates, and a tie with one of them."""
    _, _, _, latest = GG.channel_gate(date, msg, P, K, LO - 1, keep,
                                      kept_of(keep, K, P))
    mid = int(np.sort(latest)[K // 2])
    return [LO - 1, HI, -(1 << 40), 1 << 40, mid, mid - 1]


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("K", KS)
def test_kernels_match_the_oracle(K, P):
    date, msg, masks = arrays(K, P)
    batch = fake_batch(date, msg, K, P)[0]
    for name, keep in masks.items():
        for recency in recencies(date, msg, K, P, keep):
            keep2, kept2, active, latest = check_gate(
                date, msg, K, P, keep, recency, batch)
            if recency < LO:
                # nothing is older than the cutoff: keep is untouched
                assert active.all() and (keep2 == keep).all(), name
            if recency >= HI:
                assert not active.any() and not keep2.any(), name
                assert not kept2.any()
        # the tie: the channel whose newest date is the cutoff is inactive
        mid = recencies(date, msg, K, P, keep)[4]
        _, _, active, latest = GG.channel_gate(
            date, msg, P, K, mid, keep, kept_of(keep, K, P))
        assert (active[latest == mid] == 0).all() and (latest == mid).any()


@pytest.mark.parametrize("K,P", [(9, 65), (5, 130)])
def test_one_block_strides_over_the_channels(monkeypatch, K, P):
    seen = force_grid_one(monkeypatch, {"crawl_channel_gate",
                                        "crawl_compact_rows"})
    date, msg, masks = arrays(K, P)
    keep = masks["some-empty"]
    mid = recencies(date, msg, K, P, keep)[4]
    want = check_gate(date, msg, K, P, keep, mid)
    assert want[2].any() and not want[2].all()
    assert set(seen) == {"crawl_channel_gate", "crawl_compact_rows"}


@pytest.mark.parametrize("keep,recency,want_active,want_latest", HAND_CASES)
def test_hand_built_arrays(keep, recency, want_active, want_latest):
    keep = np.array(keep, dtype=np.uint8)
    _, _, active, latest = check_gate(HAND_DATE, HAND_MSG, HAND_K, HAND_P,
                                      keep, recency)
    assert active.tolist() == want_active
    assert latest.tolist() == want_latest


@pytest.mark.parametrize("K,P", [(5, 130), (9, 64)])
def test_keep_from_the_window_kernel_with_sampling(K, P):
    from crawler_amd.ops import gpu

    date, msg, _ = arrays(K, P)
    batch, chat = fake_batch(date, msg, K, P)
    kw = dict(stop_below=LO + 100, skip_above=HI - 100, cap=40, sample_k=7,
              seed=5)
    keep_t, kept_t = gpu.fetch_window(batch, **kw)
    keep, kept = GW.fetch_window(date, chat, msg, P, K, **kw)
    assert keep_t.cpu().numpy().tolist() == keep.tolist()
    assert kept.max() == 7
    for recency in recencies(date, msg, K, P, keep)[4:]:
        want = GG.channel_gate(date, msg, P, K, recency, keep, kept)
        k2 = keep_t.clone()
        n2 = kept_t.clone()
        _, _, active, latest = gpu.channel_gate(batch, k2, n2, recency,
                                                _poison=0xFF)
        got = (k2, n2, active, latest)
        for g, w in zip(got, want):
            assert g.cpu().numpy().tolist() == w.tolist()
        rows, chan = gpu.compact_rows(batch, k2, n2, _poison=0xFF)
        wr, wc = GG.compact_rows(want[0], want[1], P, K)
        assert rows.cpu().numpy().tolist() == wr.tolist()
        assert chan.cpu().numpy().tolist() == wc.tolist()
        assert want[2].any() and not want[2].all()


def test_nothing_kept_and_no_channels_launch_nothing(monkeypatch):
    from crawler_amd.ops import gpu

    K, P = 4, 65
    date, msg, masks = arrays(K, P)
    batch = fake_batch(date, msg, K, P)[0]
    keep_t = torch.zeros(K * P, dtype=torch.uint8, device=DEV)
    kept_t = torch.zeros(K, dtype=torch.int32, device=DEV)
    empty = fake_batch(date[:0], msg[:0], 0, P)[0]
    e_keep = torch.zeros(0, dtype=torch.uint8, device=DEV)
    e_kept = torch.zeros(0, dtype=torch.int32, device=DEV)
    forbid_launches(monkeypatch)
    rows, chan = gpu.compact_rows(batch, keep_t, kept_t)
    assert rows.shape == (0,) and rows.dtype == torch.int64
    assert chan.shape == (0,) and chan.dtype == torch.int32
    rows, chan = gpu.compact_rows(empty, e_keep, e_kept)
    assert rows.numel() == 0 and chan.numel() == 0
    _, _, active, latest = gpu.channel_gate(empty, e_keep, e_kept, 5)
    assert active.numel() == 0 and latest.numel() == 0


def test_drivers_check_their_arguments():
    from crawler_amd.ops import gpu

    K, P = 4, 65
    date, msg, masks = arrays(K, P)
    batch = fake_batch(date, msg, K, P)[0]
    keep_t = torch.zeros(K * P, dtype=torch.uint8, device=DEV)
    kept_t = torch.zeros(K, dtype=torch.int32, device=DEV)
    for bad_keep, bad_kept in [
        (keep_t.cpu(), kept_t),                       # wrong device
        (keep_t, kept_t.to(torch.int64)),             # wrong dtype
        (keep_t[:-1], kept_t),                        # wrong size
        (torch.zeros(2 * K * P, dtype=torch.uint8, device=DEV)[::2],
         kept_t),                                     # not contiguous
    ]:
        with pytest.raises(AssertionError):
            gpu.channel_gate(batch, bad_keep, bad_kept, 0)
        with pytest.raises(AssertionError):
            gpu.compact_rows(batch, bad_keep, bad_kept)
    with pytest.raises(ValueError):
        gpu.compact_rows(batch, keep_t, kept_t - 1)
