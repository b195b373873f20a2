"""The fetch-window kernel (csrc/fetch_window.hip) against its oracle
(ops/golden_window.py): hand-built date tensors around every tile edge,
caps, sample sizes and seeds; what it writes and what it leaves alone; and
the window -> select_rows -> parse_encode chain against the CPU encoder."""
import functools
import types

import numpy as np
import pytest
import torch

from _corpora import NOW, forbid_launches, force_grid_one
from crawler_amd.ops import batch as B
from crawler_amd.ops import golden_window as GW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LO, HI = 1000, 2000
KS = [1, 4, 5, 9]
PS = [1, 2, 63, 64, 65, 129, 257]
SEEDS = [0, 123, -1, 2 ** 63 - 1, 2 ** 63]
KEY_SLOTS = 1024   # fetch_window.hip: keys a wave holds in LDS


def ids(K, P):
    """Distinct (chat_id, msg_id) per row, as the synthetic feed lays
    them out."""
    chat = np.repeat(-(1001000000000 + 3 * np.arange(K, dtype=np.int64) + 1),
                     P)
    msg = np.tile((np.arange(P, dtype=np.int64) + 1) << 20, K)
    return chat, msg


def fake_batch(date, K, P, device=DEV):
    """The fields fetch_window reads, on the device."""
    chat, msg = ids(K, P)
    t = lambda a, dt_: torch.tensor(np.asarray(a), dtype=dt_, device=device)
    return types.SimpleNamespace(
        device=torch.device(device), n=K * P, n_channels=K,
        meta={"date": t(date, torch.int32)},
        chat_id=t(chat, torch.int64), msg_id=t(msg, torch.int64))


def at_walk(d, P, c, w, value):
    """Set the row ``w`` steps into channel c's newest-first walk."""
    if 0 <= w < P:
        d[c * P + P - 1 - w] = value


@functools.lru_cache(maxsize=None)
def patterns(K, P):
    """{name: int32[K*P]} of hand-built dates; stop_below = LO,
    skip_above = HI."""
    rng = np.random.default_rng(1000 * K + P)
    inside = lambda: (LO + (np.arange(K * P) % P) * 900 // P).astype(np.int32)
    out = {"monotone": inside()}
    d = inside()
    for c in range(K):                      # the dip is the newest row,
        at_walk(d, P, c, c % 2, LO - 1)     # or the one behind it
    out["dip-newest"] = d
    d = inside()
    for c in range(K):                      # in the middle of a tile
        at_walk(d, P, c, 20 + c, LO - 1)
        at_walk(d, P, c, 90 + c, LO - 1)
    out["dip-mid-tile"] = d
    d = inside()
    for c in range(K):                      # last lane / first lane of a tile
        at_walk(d, P, c, (63, 64, 127, 128)[c % 4], LO - 1)
    out["dip-tile-edge"] = d
    out["all-above"] = np.full(K * P, HI + 1, dtype=np.int32)
    out["all-below"] = np.full(K * P, LO - 1, dtype=np.int32)
    cyc = np.array([LO, HI, HI + 1, LO + 1, HI - 1, HI + 1, HI + 1],
                   dtype=np.int32)
    d = cyc[np.arange(K * P) % 7].copy()
    for c in range(K):
        at_walk(d, P, c, 100 + 9 * c, LO - 1)
    out["ties"] = d
    # no order at all: above, inside and (rarely) below
    d = rng.integers(LO, HI + 400, K * P).astype(np.int32)
    d[rng.random(K * P) < 0.01] = LO - 1
    out["random"] = d
    return out


def run(batch, **kw):
    from crawler_amd.ops import gpu

    res = gpu.fetch_window(batch, **kw)
    keep, kept = res
    assert keep.dtype == torch.uint8 and kept.dtype == torch.int32
    return keep.cpu().numpy(), kept.cpu().numpy(), res


def oracle(date, K, P, **kw):
    chat, msg = ids(K, P)
    return GW.fetch_window(date, chat, msg, P, K, **kw)


def check(date, K, P, batch=None, **kw):
    batch = batch or fake_batch(date, K, P)
    keep, kept, _ = run(batch, **kw)
    want_keep, want_kept = oracle(date, K, P, **kw)
    assert kept.tolist() == want_kept.tolist(), kw
    bad = np.nonzero(keep != want_keep)[0]
    assert bad.size == 0, (kw, bad[:8].tolist())
    return want_kept


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("K", KS)
def test_kernel_matches_the_oracle(K, P):
    pairs = set()
    for pi, (name, date) in enumerate(patterns(K, P).items()):
        batch = fake_batch(date, K, P)
        for ci, cap in enumerate([0, 1, 63, 64, 65, P]):
            # candidates of channel 0 before sampling
            _, n0 = oracle(date[:P], 1, P, stop_below=LO, skip_above=HI,
                           cap=cap)
            cand = int(n0[0])
            # the sample size and the seed rotate against the cap and
            # the pattern, so that all 30 pairs of them come up
            si, ei = (ci + pi) % 6, (pi + 2 * ci) % 5
            sample_k = max([0, 1, 2, cand - 1, cand, cand + 1][si], 0)
            seed = SEEDS[ei]
            pairs.add((si, ei))
            check(date, K, P, batch=batch, stop_below=LO, skip_above=HI,
                  cap=cap, sample_k=sample_k, seed=seed)
    assert len(pairs) == 30   # every sample size with every seed


@pytest.mark.parametrize("P", [63, 64, 65, 257])
def test_unbounded_sides_and_inverted_bounds(P):
    K = 5
    pats = patterns(K, P)
    for name in ("random", "ties", "dip-mid-tile"):
        date = pats[name]
        batch = fake_batch(date, K, P)
        for kw in (dict(), dict(stop_below=LO), dict(skip_above=HI),
                   dict(cap=7), dict(stop_below=LO, sample_k=3, seed=5),
                   # everything at or below HI is below the stop: rows
                   # above HI are skipped, the first other row ends it
                   dict(stop_below=HI + 1000, skip_above=HI),
                   dict(stop_below=-2 ** 63, skip_above=2 ** 63 - 1),
                   dict(stop_below=2 ** 40, skip_above=-2 ** 40)):
            check(date, K, P, batch=batch, **kw)


def test_dates_at_the_int32_limits():
    K, P = 2, 70
    date = np.tile(np.array([-2 ** 31, 2 ** 31 - 1, 0, -1, 1], dtype=np.int64),
                   K * P // 5).astype(np.int32)
    for kw in (dict(), dict(stop_below=-2 ** 31), dict(stop_below=-2 ** 31 + 1),
               dict(skip_above=2 ** 31 - 2), dict(skip_above=2 ** 31 - 1),
               dict(stop_below=0, skip_above=0, sample_k=2)):
        check(date, K, P, **kw)


@pytest.mark.parametrize("cand", [KEY_SLOTS - 1, KEY_SLOTS, KEY_SLOTS + 1,
                                  KEY_SLOTS + 76])
def test_sample_threshold_between_lds_keys_and_recomputed_keys(cand):
    """Up to KEY_SLOTS candidates the k-th key is searched in LDS, above
    that the keys are recomputed from the rows."""
    K, P = 3, KEY_SLOTS + 80
    date = np.full(K * P, LO + 5, dtype=np.int32)
    for c in range(K):
        at_walk(date, P, c, 3, HI + 1)    # one skipped row, then channel
        at_walk(date, P, c, cand + 1 + 40 * c, LO - 1)   # 0 has cand rows
    _, n_all = oracle(date, K, P, stop_below=LO, skip_above=HI)
    assert n_all[0] == cand and n_all.min() == cand
    batch = fake_batch(date, K, P)
    for sample_k, seed in ((1, 0), (cand // 2, 123), (cand - 2, -1)):
        n = check(date, K, P, batch=batch, stop_below=LO, skip_above=HI,
                  sample_k=sample_k, seed=seed)
        assert n.tolist() == [sample_k] * K
    n = check(date, K, P, batch=batch, stop_below=LO, skip_above=HI,
              cap=KEY_SLOTS + 1, sample_k=KEY_SLOTS, seed=7)
    assert n[0] == min(cand, KEY_SLOTS)


def test_one_block_strides_over_the_channels(monkeypatch):
    K, P = 9, 129
    date = patterns(K, P)["random"]
    batch = fake_batch(date, K, P)
    kw = dict(stop_below=LO, skip_above=HI, cap=40, sample_k=11, seed=123)
    many = run(batch, **kw)
    seen = force_grid_one(monkeypatch, {"crawl_fetch_window"})
    one = run(batch, **kw)
    assert seen == ["crawl_fetch_window"]
    assert (one[0] == many[0]).all() and (one[1] == many[1]).all()
    check(date, K, P, batch=batch, **kw)


@pytest.mark.parametrize("poison", [0xA5, 0xFF])
def test_writes_all_of_its_outputs_and_nothing_else(poison):
    G = 256
    for K, P in ((1, 1), (5, 65), (9, 257)):
        for name in ("all-above", "all-below", "dip-tile-edge", "random"):
            date = patterns(K, P)[name]
            kw = dict(stop_below=LO, skip_above=HI, cap=70, sample_k=9,
                      seed=1)
            keep, kept, res = run(fake_batch(date, K, P), _poison=poison,
                                  _guard=G, **kw)
            want_keep, want_kept = oracle(date, K, P, **kw)
            # every byte rewritten: the poison is neither 0 nor 1, and no
            # count equals four poison bytes
            assert (keep == want_keep).all(), (K, P, name)
            assert (kept == want_kept).all(), (K, P, name)
            raw = res.raw_keep.cpu().numpy()
            assert raw.size == K * P + 2 * G
            assert (raw[:G] == poison).all() and (raw[-G:] == poison).all()
            rawk = res.raw_kept.cpu().numpy().view(np.uint8)
            assert rawk.size == 4 * (K + 2 * G)
            assert (rawk[:4 * G] == poison).all()
            assert (rawk[-4 * G:] == poison).all()


def test_no_channels_no_launch_and_negative_arguments(monkeypatch):
    from crawler_amd.ops import gpu

    batch = fake_batch(patterns(4, 64)["monotone"], 4, 64)
    with pytest.raises(ValueError):
        gpu.fetch_window(batch, cap=-1)
    with pytest.raises(ValueError):
        gpu.fetch_window(batch, sample_k=-1)
    empty = fake_batch(np.zeros(0, dtype=np.int32), 0, 0)
    forbid_launches(monkeypatch)
    keep, kept = gpu.fetch_window(empty, stop_below=LO, cap=3, sample_k=2)
    assert keep.shape == (0,) and keep.dtype == torch.uint8
    assert kept.shape == (0,) and kept.dtype == torch.int32
    assert keep.device.type == "cuda" and kept.device.type == "cuda"


@pytest.mark.parametrize("sample_k", [0, 7])
def test_window_select_rows_parse_encode_matches_the_cpu_chain(sample_k):
    from crawler_amd.feed import FeedConfig, SyntheticFeed
    from crawler_amd.ops import gpu
    from crawler_amd.ops.golden_batch import encode_batch

    K, P = 3, 200
    feed = SyntheticFeed(FeedConfig(seed=31, universe=500,
                                    posts_per_channel=P))
    cpu_b = feed.build_batch(np.array([3, 9, 17]), posts_per_channel=P)
    base, step = feed.cfg.base_date, feed.cfg.date_step
    lo, hi = base + 50 * step, base + 150 * step
    date = cpu_b.meta["date"]
    date[P + 120] = lo - 1            # channel 1 ends early
    date[2 * P + 130:2 * P + 140] = hi + 5   # channel 2: skipped inside
    kw = dict(stop_below=lo, skip_above=hi, cap=90, sample_k=sample_k,
              seed=9)
    want_keep, want_kept = GW.fetch_window(
        date.numpy(), cpu_b.chat_id.numpy(), cpu_b.msg_id.numpy(), P, K, **kw)
    if sample_k:
        assert want_kept.tolist() == [sample_k] * K
    else:
        assert want_kept.min() > 0 and len(set(want_kept.tolist())) > 1
    dev_b = cpu_b.to(DEV)
    keep, kept = gpu.fetch_window(dev_b, **kw)
    assert (keep.cpu().numpy() == want_keep).all()
    assert kept.cpu().tolist() == want_kept.tolist()
    res = gpu.parse_encode(B.select_rows(dev_b, keep.nonzero().flatten()),
                           now=NOW)
    rows = np.nonzero(want_keep)[0]
    lines, _ = encode_batch(B.select_rows(cpu_b, torch.from_numpy(rows)),
                            now=NOW)
    assert len(lines) == int(want_kept.sum())
    assert bytes(res.out.cpu().numpy()) == b"".join(lines)
    # the subset's lines are the full batch's lines at those rows
    full, _ = encode_batch(cpu_b, now=NOW)
    assert lines == [full[r] for r in rows]
