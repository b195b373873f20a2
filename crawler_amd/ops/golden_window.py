"""Python oracle of the fetch-window kernel (csrc/fetch_window.hip).

Which rows of a K x P channel-grouped batch the crawl keeps: the walk of
``engine.pipeline.fetch_channel_messages`` (telegramutils.go:25-157) over
rows instead of pages, with the GPU path's sampling rule in place of the
Fisher-Yates shuffle. A channel's rows are stored oldest first, so the
newest-first walk is descending row index; nothing here looks at
``msg_id`` order or assumes that dates are monotone.

Sampling keeps the ``sample_k`` candidates with the smallest

    key(r) = splitmix64(seed ^ (chat_id[r] * 0x9E3779B97F4A7C15 + msg_id[r]))

in uint64 arithmetic. Precondition: ``(chat_id, msg_id)`` is distinct
within a channel; splitmix64 is a bijection, so the keys are distinct too
and there are no ties. The keys behave like i.i.d. draws, so the k
smallest are a uniform sample without replacement, and they depend only
on the message's identity and the seed, never on where the channel sits
in a batch.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

_M64 = (1 << 64) - 1
NO_STOP = -(1 << 62)   # stop_below when no lower bound is set
NO_SKIP = 1 << 62      # skip_above when no upper bound is set


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample_key(seed: int, chat_id: int, msg_id: int) -> int:
    ident = ((chat_id & _M64) * 0x9E3779B97F4A7C15 + (msg_id & _M64)) & _M64
    return splitmix64((seed & _M64) ^ ident)


def window_rows(dates: Sequence[int], chat_ids: Sequence[int],
                msg_ids: Sequence[int], stop_below: Optional[int] = None,
                skip_above: Optional[int] = None, cap: int = 0,
                sample_k: int = 0, seed: int = 0) -> List[int]:
    """Kept row indices of ONE channel (rows oldest first), ascending."""
    lo = NO_STOP if stop_below is None else stop_below
    hi = NO_SKIP if skip_above is None else skip_above
    cand = []
    for r in range(len(dates) - 1, -1, -1):
        d = int(dates[r])
        if d > hi:
            continue
        if d < lo:
            break
        cand.append(r)
        if cap > 0 and len(cand) >= cap:
            break
    if sample_k > 0 and len(cand) > sample_k:
        cand.sort(key=lambda r: sample_key(seed, int(chat_ids[r]),
                                           int(msg_ids[r])))
        cand = cand[:sample_k]
    return sorted(cand)


def fetch_window(date, chat_id, msg_id, P: int, K: int,
                 stop_below: Optional[int] = None,
                 skip_above: Optional[int] = None, cap: int = 0,
                 sample_k: int = 0,
                 seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(keep uint8[K*P], kept int32[K]) of a K x P batch: what
    ``gpu.fetch_window`` returns."""
    date = np.asarray(date).reshape(-1)
    chat_id = np.asarray(chat_id).reshape(-1)
    msg_id = np.asarray(msg_id).reshape(-1)
    assert date.size == chat_id.size == msg_id.size == K * P
    keep = np.zeros(K * P, dtype=np.uint8)
    kept = np.zeros(K, dtype=np.int32)
    for c in range(K):
        s = slice(c * P, (c + 1) * P)
        rows = window_rows(date[s], chat_id[s], msg_id[s], stop_below,
                           skip_above, cap, sample_k, seed)
        keep[c * P + np.asarray(rows, dtype=np.int64)] = 1
        kept[c] = len(rows)
    return keep, kept
