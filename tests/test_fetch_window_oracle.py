"""The fetch-window oracle (ops/golden_window.py) against the CPU crawl's
fetch_channel_messages, gpu.window_params against the CPU precedence
rules, and the sampling rule's own properties. CPU only."""
import datetime as dt
import math
import random

import numpy as np
import pytest

from crawler_amd.config import CrawlerConfig
from crawler_amd.engine.pipeline import fetch_channel_messages
from crawler_amd.ops import golden_window as GW
from crawler_amd.ops import gpu

UTC = dt.timezone.utc
LO, HI = 1000, 2000
PS = [1, 99, 100, 101, 250]


def ts(x):
    return dt.datetime.fromtimestamp(x, UTC)


class _Msg:
    def __init__(self, msg_id, date):
        self.msg_id, self.date = msg_id, date


class StubClient:
    """One channel, rows oldest first; pages newest first, 100 a page."""

    def __init__(self, dates):
        self.msgs = [_Msg((r + 1) << 20, int(d)) for r, d in enumerate(dates)]
        self.pages = 0

    def get_chat_history(self, chat_id, from_message_id=0, limit=100):
        self.pages += 1
        out = self.msgs[::-1]
        if from_message_id:
            out = [m for m in out if m.msg_id < from_message_id]
        return out[:min(limit, 100)]


def _monotone(P):
    return [LO - 100 + (1200 * r) // P for r in range(P)]


def _shuffled(P):
    d = _monotone(P)
    random.Random(P).shuffle(d)
    return d


def _above_interleaved(P):
    # every row at or above LO; one in three above HI
    rng = random.Random(100 + P)
    return [HI + rng.randint(1, 50) if rng.random() < 0.33
            else rng.randint(LO, HI) for _ in range(P)]


def _dip(P):
    # all inside, but one row below LO with in-window rows behind it
    d = [LO + 1 + (r % 900) for r in range(P)]
    d[P // 2] = LO - 1
    return d


def _dip_newest(P):
    d = [LO + 1 + (r % 900) for r in range(P)]
    d[P - 1] = LO - 1
    return d


def _ties(P):
    cyc = [LO, HI, LO + 1, HI - 1, HI + 1]
    d = [cyc[r % 5] for r in range(P)]
    if P > 3:
        d[P // 3] = LO - 1
    return d


def _stop_after_first_page(P):
    # the stop is the first row of the second page
    d = [LO + 5] * P
    if P > 100:
        d[P - 101] = LO - 1
    return d


def _stop_ends_first_page(P):
    # the stop is the last row of the first page
    d = [LO + 5] * P
    if P >= 100:
        d[P - 100] = LO - 1
    return d


def _all_above(P):
    return [HI + 1 + r for r in range(P)]


def _all_below(P):
    return [LO - 1 - r for r in range(P)]


PATTERNS = [_monotone, _shuffled, _above_interleaved, _dip, _dip_newest,
            _ties, _stop_after_first_page, _stop_ends_first_page,
            _all_above, _all_below]

# (name, config keywords): date-between, min_post_date alone, one
# date-between bound with min_post_date, no bound, fractional bounds
BOUNDS = [
    ("between", dict(date_between_min=ts(LO), date_between_max=ts(HI))),
    ("between-overrides", dict(date_between_min=ts(LO),
                               date_between_max=ts(HI),
                               min_post_date=ts(HI - 100))),
    ("min-post-date", dict(min_post_date=ts(LO))),
    ("one-bound", dict(date_between_max=ts(HI), min_post_date=ts(LO))),
    ("none", dict()),
    ("fractional", dict(date_between_min=ts(LO - 0.5),
                        date_between_max=ts(HI + 0.5))),
    ("fractional-in", dict(date_between_min=ts(LO + 0.25),
                           date_between_max=ts(HI - 0.25))),
]


def _oracle_ids(cfg, dates):
    """msg_ids the oracle keeps under window_params(cfg); with no params
    the GPU crawl's per-row rule (all rows at or after min_post_date)."""
    P = len(dates)
    ids = [(r + 1) << 20 for r in range(P)]
    params = gpu.window_params(cfg)
    if params is None:
        return None
    rows = GW.window_rows(dates, [-1001] * P, ids, **params)
    return {ids[r] for r in rows}


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda f: f.__name__)
def test_oracle_keeps_what_fetch_channel_messages_returns(pattern, P):
    dates = pattern(P)
    checked = 0
    for name, kw in BOUNDS:
        for cap in (0, 1, 100, P):
            cfg = CrawlerConfig(max_posts=cap, **kw)
            want = _oracle_ids(cfg, dates)
            if want is None:
                # nothing for the window kernel to do
                assert cap == 0 and name in ("min-post-date", "one-bound",
                                             "none")
                continue
            got = fetch_channel_messages(StubClient(dates), -1001, cfg)
            assert len(got) == len({m.msg_id for m in got})
            assert {m.msg_id for m in got} == want, (name, cap)
            checked += 1
    assert checked >= 4 * 4 + 3 * 3


def test_patterns_hold_what_they_promise():
    for P in PS:
        d = _dip(P)
        assert d[P // 2] < LO
        if P > 2:
            assert all(LO <= x <= HI for x in d[:P // 2])
        t = _ties(P)
        if P >= 5:
            assert LO in t and HI in t and HI + 1 in t
        a = _above_interleaved(P)
        assert min(a) >= LO
        if P >= 99:
            # interleaved: a skipped row with kept rows on both sides
            above = "".join("a" if x > HI else "i" for x in a)
            assert "ia" in above and "ai" in above
    # the walk ends at a dip even though older rows are inside again
    rows = GW.window_rows(_dip(101), [-1] * 101, list(range(101)), LO, HI)
    assert rows == list(range(51, 101))
    # stops and caps on page edges
    c = StubClient(_stop_after_first_page(250))
    cfg = CrawlerConfig(date_between_min=ts(LO), date_between_max=ts(HI))
    assert len(fetch_channel_messages(c, -1, cfg)) == 100 and c.pages == 2
    c = StubClient(_stop_ends_first_page(250))
    assert len(fetch_channel_messages(c, -1, cfg)) == 99 and c.pages == 1


# ------------------------------------------------------------ window_params

def test_window_params_default_and_min_post_date_only_are_none():
    assert gpu.window_params(CrawlerConfig()) is None
    assert gpu.window_params(CrawlerConfig(min_post_date=ts(LO))) is None
    assert gpu.window_params(CrawlerConfig(min_post_date=ts(LO),
                                           max_posts=0)) is None
    assert gpu.window_params(CrawlerConfig(min_post_date=ts(LO),
                                           max_posts=-1)) is None
    # sample_size alone is not a sampling request (_maybe_sample)
    assert gpu.window_params(CrawlerConfig(min_post_date=ts(LO),
                                           sample_size=5)) is None


def test_window_params_date_between_overrides_min_post_date():
    p = gpu.window_params(CrawlerConfig(
        date_between_min=ts(LO), date_between_max=ts(HI),
        min_post_date=ts(HI - 1)))
    assert (p["stop_below"], p["skip_above"]) == (LO, HI)
    assert p["cap"] == 0 and p["sample_k"] == 0 and p["seed"] == 0


def test_window_params_one_bound_uses_min_post_date():
    p = gpu.window_params(CrawlerConfig(
        date_between_max=ts(HI), min_post_date=ts(LO), max_posts=3))
    assert (p["stop_below"], p["skip_above"], p["cap"]) == (LO, None, 3)
    p = gpu.window_params(CrawlerConfig(
        date_between_min=ts(LO + 7), min_post_date=ts(LO), max_posts=3))
    assert (p["stop_below"], p["skip_above"]) == (LO, None)
    p = gpu.window_params(CrawlerConfig(date_between_min=ts(LO),
                                        max_posts=3))
    assert (p["stop_below"], p["skip_above"]) == (None, None)


def test_window_params_sampling_needs_date_between_min():
    both = dict(date_between_min=ts(LO), date_between_max=ts(HI))
    assert gpu.window_params(CrawlerConfig(sample_size=9,
                                           **both))["sample_k"] == 9
    assert gpu.window_params(CrawlerConfig(sample_size=0,
                                           **both))["sample_k"] == 0
    p = gpu.window_params(CrawlerConfig(sample_size=9, max_posts=4,
                                        date_between_max=ts(HI)))
    assert p["sample_k"] == 0 and p["cap"] == 4
    # date_between_min alone is enough for _maybe_sample
    p = gpu.window_params(CrawlerConfig(sample_size=9,
                                        date_between_min=ts(LO)))
    assert p["sample_k"] == 9 and p["stop_below"] is None
    p = gpu.window_params(CrawlerConfig(sample_size=9, sample_seed=77,
                                        **both))
    assert p["seed"] == 77


def test_window_params_max_posts_zero_or_negative_is_no_cap():
    both = dict(date_between_min=ts(LO), date_between_max=ts(HI))
    for mp in (-1, 0):
        assert gpu.window_params(CrawlerConfig(max_posts=mp,
                                               **both))["cap"] == 0
    assert gpu.window_params(CrawlerConfig(max_posts=1))["cap"] == 1


@pytest.mark.parametrize("frac", [0.0, 0.001, 0.5, 0.999])
def test_window_params_fractional_bounds_compare_like_the_cpu(frac):
    lo, hi = ts(LO + frac), ts(HI + frac)
    p = gpu.window_params(CrawlerConfig(date_between_min=lo,
                                        date_between_max=hi))
    assert p["stop_below"] == math.ceil(lo.timestamp())
    assert p["skip_above"] == math.floor(hi.timestamp())
    for d in range(LO - 1, LO + 3):
        assert (d < p["stop_below"]) == (d < lo.timestamp())
    for d in range(HI - 1, HI + 3):
        assert (d > p["skip_above"]) == (d > hi.timestamp())
    p = gpu.window_params(CrawlerConfig(min_post_date=lo, max_posts=1))
    for d in range(LO - 1, LO + 3):
        assert (d < p["stop_below"]) == (d < lo.timestamp())


# ----------------------------------------------------------------- sampling

def _channels(K, P, seed=5):
    """K channels of P rows: dates inside, above and (rarely) below the
    window, in no order."""
    rng = random.Random(seed)
    date = [rng.choice([LO, LO + 3, HI, HI - 7, HI + 2, LO - 1]
                       if rng.random() < 0.05 else [rng.randint(LO, HI + 99)])
            for _ in range(K * P)]
    chat = [-(1001000000000 + 17 * c) for c in range(K) for _ in range(P)]
    msg = [(p + 1) << 20 for _ in range(K) for p in range(P)]
    return np.array(date), np.array(chat), np.array(msg)


def test_sample_size_subset_and_determinism():
    K, P = 12, 70
    date, chat, msg = _channels(K, P)
    full, n_full = GW.fetch_window(date, chat, msg, P, K, LO, HI)
    assert 0 < n_full.min() and len(set(n_full.tolist())) > 1
    for k in (1, 2, int(n_full.min()), int(n_full.max()), P + 1):
        keep, kept = GW.fetch_window(date, chat, msg, P, K, LO, HI,
                                     sample_k=k, seed=3)
        assert kept.tolist() == np.minimum(k, n_full).tolist()
        assert keep.reshape(K, P).sum(axis=1).tolist() == kept.tolist()
        assert not (keep & ~full & 1).any()          # a subset
        again, _ = GW.fetch_window(date, chat, msg, P, K, LO, HI,
                                   sample_k=k, seed=3)
        assert (again == keep).all()
    a, _ = GW.fetch_window(date, chat, msg, P, K, LO, HI, sample_k=5, seed=0)
    b, _ = GW.fetch_window(date, chat, msg, P, K, LO, HI, sample_k=5,
                           seed=123)
    assert (a != b).any()
    # the cap comes first, the sample is drawn from the capped walk
    capped, n_cap = GW.fetch_window(date, chat, msg, P, K, LO, HI, cap=9)
    assert n_cap.max() == 9
    both, n = GW.fetch_window(date, chat, msg, P, K, LO, HI, cap=9,
                              sample_k=4, seed=1)
    assert n.tolist() == np.minimum(4, n_cap).tolist()
    assert not (both & ~capped & 1).any()


def test_sample_does_not_depend_on_the_channels_place_in_a_batch():
    K, P = 7, 40
    date, chat, msg = _channels(K, P, seed=8)
    keep, kept = GW.fetch_window(date, chat, msg, P, K, LO, HI, sample_k=6,
                                 seed=42)
    keep = keep.reshape(K, P)
    order = [3, 0, 6, 5, 1, 4, 2]
    sel = np.concatenate([np.arange(c * P, (c + 1) * P) for c in order])
    keep2, kept2 = GW.fetch_window(date[sel], chat[sel], msg[sel], P, K, LO,
                                   HI, sample_k=6, seed=42)
    assert (keep2.reshape(K, P) == keep[order]).all()
    assert kept2.tolist() == kept[order].tolist()
    for c in range(K):
        s = slice(c * P, (c + 1) * P)
        one, n1 = GW.fetch_window(date[s], chat[s], msg[s], P, 1, LO, HI,
                                  sample_k=6, seed=42)
        assert (one == keep[c]).all() and n1[0] == kept[c]


def test_sample_key_is_the_documented_function():
    m = (1 << 64) - 1
    for seed, chat, msg in [(0, -1001000000000, 1 << 20),
                            (123, -1001000000499, 64 << 20),
                            (-1, -5, 7), (2 ** 63, 0, 0),
                            (2 ** 63 - 1, 2 ** 62, 2 ** 62)]:
        ident = ((chat % 2 ** 64) * 0x9E3779B97F4A7C15 + msg % 2 ** 64) & m
        x = (seed % 2 ** 64) ^ ident
        z = (x + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        assert GW.sample_key(seed, chat, msg) == z ^ (z >> 31)
    # the splitmix64 of the reservoir oracle's stream
    assert GW.splitmix64(0) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("seed", [0, 123])
@pytest.mark.parametrize("P,k", [(8, 2), (5, 1)])
def test_sample_is_uniform_over_row_positions(P, k, seed):
    """Over 2000 channels every row position is drawn K*k/P times, give
    or take 4 binomial standard deviations."""
    K = 2000
    chat = np.repeat(-(1001000000000 + np.arange(K, dtype=np.int64)), P)
    msg = np.tile((np.arange(P, dtype=np.int64) + 1) << 20, K)
    keep, kept = GW.fetch_window(np.zeros(K * P, dtype=np.int32), chat, msg,
                                 P, K, sample_k=k, seed=seed)
    assert kept.tolist() == [k] * K
    counts = keep.reshape(K, P).sum(axis=0)
    p = k / P
    sd = math.sqrt(K * p * (1 - p))
    dev = np.abs(counts - K * p) / sd
    print("P=%d k=%d seed=%d worst deviation %.2f sd" % (P, k, seed,
                                                         dev.max()))
    assert dev.max() <= 4.0
