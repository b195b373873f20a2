"""Cases for the channel gate that the oracle tests, the kernel tests and
the engine tests share."""
import numpy as np

# Two channels of five rows, dates not monotone, the greatest msg_id in
# neither channel's last row (GPU tests reuse these arrays).
HAND_P, HAND_K = 5, 2
HAND_DATE = np.array([50, 90, 70, 95, 60,   80, 20, 99, 40, 30],
                     dtype=np.int32)
HAND_MSG = np.array([5, 9, 7, 3, 1,   2, 11, 4, 6, 8], dtype=np.int64)
HAND_CASES = [
    # (keep, recency, expected active, expected latest)
    # nothing kept: the row with the greatest msg_id decides (90 / 20)
    ([0] * 10, 50, [1, 0], [90, 20]),
    ([0] * 10, 90, [0, 0], [90, 20]),
    ([0] * 10, 19, [1, 1], [90, 20]),
    # a sample-like mask: the greatest kept date, not the last kept row
    ([1, 0, 1, 0, 1,   0, 1, 0, 1, 1], 60, [1, 0], [70, 40]),
    ([1, 0, 1, 0, 1,   0, 1, 0, 1, 1], 39, [1, 1], [70, 40]),
    # one channel kept, one not; ties on both sides
    ([0, 0, 0, 1, 0,   0, 0, 0, 0, 0], 95, [0, 0], [95, 20]),
    ([0, 0, 0, 1, 0,   0, 0, 0, 0, 0], 94, [1, 0], [95, 20]),
    ([1, 1, 1, 1, 1,   1, 1, 1, 1, 1], 98, [0, 1], [95, 99]),
]


_splits = {}


def split_channels(feed, P, n=6):
    """``n`` channel ids and a cutoff inside the 30-second band of the
    newest posts: the cutoff is the newest date of one of them (a tie),
    and channels lie on both sides of it."""
    key = (repr(feed.cfg), P, n)
    if key not in _splits:
        _splits[key] = _split_channels(feed, P, n)
    return _splits[key]


def _split_channels(feed, P, n):
    cand = list(range(1, 40))
    b = feed.build_batch(np.array(cand), posts_per_channel=P)
    dates = b.meta["date"].numpy().reshape(len(cand), P)
    newest = dates.max(axis=1)
    order = np.argsort(newest, kind="stable")
    tie = order[len(order) // 2]
    cutoff = int(newest[tie])
    above = [c for c, d in zip(cand, newest) if d > cutoff]
    below = [c for c, d in zip(cand, newest) if d < cutoff]
    assert above and below
    half = (n - 1) // 2
    cids = sorted([cand[tie]] + above[:half] + below[:n - 1 - half])
    return cids, cutoff, cand[tie]
