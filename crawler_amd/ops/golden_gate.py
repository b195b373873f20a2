"""Python oracle of the channel gate and the kept-row compaction
(csrc/channel_gate.hip).

The gate is the activity deadend of ``engine.pipeline.run_for_channel``
(runner.go:628-643) over the rows of a K x P channel-grouped batch whose
fetch window (``golden_window.fetch_window``) is already known:

- a channel that fetched messages takes ``max(m.date for m in messages)``,
  the newest of the FETCHED list, after cap and sampling;
- a channel that fetched none asks ``get_chat_history(limit=1)`` for the
  chat's newest message, the one with the greatest ``msg_id``, and takes
  its date;
- ``is_channel_active``: active iff that date is later than the cutoff
  (``latest_ts <= cutoff`` is inactive, so a tie is inactive). Dates are
  integers, so ``d > cutoff`` is ``d > floor(cutoff)``.

An inactive channel is a deadend: it writes no post and none of its links
is followed, so its rows leave the kept set. Nothing here assumes that
dates are monotone or that the newest message is the last row.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np


def channel_gate(date, msg_id, P: int, K: int, recency: int, keep,
                 kept) -> Tuple[np.ndarray, np.ndarray, np.ndarray,
                                np.ndarray]:
    """(keep uint8[K*P], kept int32[K], active uint8[K], latest int32[K])
    after the gate; the inputs are left as they are."""
    date = np.asarray(date).reshape(-1)
    msg_id = np.asarray(msg_id).reshape(-1)
    keep = np.array(keep, dtype=np.uint8).reshape(-1)
    kept = np.array(kept, dtype=np.int32).reshape(-1)
    assert date.size == msg_id.size == keep.size == K * P and kept.size == K
    assert P >= 1 or K == 0
    active = np.zeros(K, dtype=np.uint8)
    latest = np.zeros(K, dtype=np.int32)
    for c in range(K):
        rows = range(c * P, (c + 1) * P)
        if kept[c] > 0:
            fetched = [int(date[r]) for r in rows if keep[r]]
            newest = max(fetched)
        else:
            # of equal msg_ids (outside the precondition) the first row
            top = max(rows, key=lambda r: (int(msg_id[r]), -r))
            newest = int(date[top])
        latest[c] = newest
        active[c] = 1 if newest > recency else 0
        if not active[c]:
            keep[c * P:(c + 1) * P] = 0
            kept[c] = 0
    return keep, kept, active, latest


def compact_rows(keep, kept, P: int, K: int) -> Tuple[np.ndarray,
                                                      np.ndarray]:
    """(rows int64[sum(kept)], row_channel int32[sum(kept)]): the global
    indices of the kept rows, channel by channel and ascending within
    one, and each row's channel."""
    keep = np.asarray(keep).reshape(-1)
    kept = np.asarray(kept).reshape(-1)
    assert keep.size == K * P and kept.size == K
    rows, chans = [], []
    for c in range(K):
        mine = [r for r in range(c * P, (c + 1) * P) if keep[r]]
        assert len(mine) == int(kept[c]), f"channel {c}: keep/kept differ"
        rows += mine
        chans += [c] * len(mine)
    return (np.asarray(rows, dtype=np.int64),
            np.asarray(chans, dtype=np.int32))
