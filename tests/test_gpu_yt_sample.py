"""yt_sample.hip kernels vs the synthetic index's own Python: search,
first-claim, uploads, and the batch builder (yt_feedgen.hip) on their ids."""
import datetime as dt
import random

import numpy as np
import pytest
import torch

from crawler_amd.youtube.batch import encode_yt_batch, pack_videos
from crawler_amd.youtube.client import SyntheticYouTubeClient
from crawler_amd.youtube.synth import SyntheticYouTubeIndex

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NOW = dt.datetime(2026, 3, 4, 5, 6, 7, tzinfo=dt.timezone.utc)
valid_rule = SyntheticYouTubeClient.is_valid_sample


def _index():
    return SyntheticYouTubeIndex(seed=5, universe_channels=3000)


def _prefix_tensor(prefixes):
    a = np.frombuffer("".join(prefixes).encode(), dtype=np.uint8)
    return torch.from_numpy(a.copy().reshape(len(prefixes), 5)).to(DEV)


def _ids_tensor(ids):
    a = np.frombuffer("".join(ids).encode(), dtype=np.uint8)
    return torch.from_numpy(a.copy().reshape(len(ids), 11)).to(DEV)


def _search_host(prefixes):
    from crawler_amd.ops import gpu

    r = gpu.yt_search(_index(), _prefix_tensor(prefixes))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check_search(prefixes):
    from crawler_amd.ops import gpu

    idx = _index()
    r = _search_host(prefixes)
    S = len(prefixes)
    W = gpu.YT_SEARCH_SLOTS
    assert r["ids"].shape == (S, W, 11) and r["flags"].shape == (S, W)
    chan = r["chan"].reshape(S, W)
    vcount = r["vcount"].reshape(S, W)
    for s, prefix in enumerate(prefixes):
        want = idx.search_prefix(prefix)
        assert len(want) <= W
        for j in range(W):
            f = int(r["flags"][s, j])
            if j >= len(want):
                assert f == 0, (prefix, j)
                continue
            got = bytes(r["ids"][s, j]).decode()
            assert got == want[j], (prefix, j)
            ok = valid_rule(want[j], prefix)
            assert f == (1 | (2 if ok else 0)), (prefix, j)
            if ok:
                v = idx.video(want[j])
                n = idx.channel_index_of(v.channel_id)
                assert int(chan[s, j]) == n
                assert int(vcount[s, j]) == idx.channel(n).video_count
    return r


def test_search_empty():
    from crawler_amd.ops import gpu

    r = gpu.yt_search(_index(), torch.zeros((0, 5), dtype=torch.uint8,
                                            device=DEV))
    assert r["ids"].shape == (0, 17, 11) and r["keys"].numel() == 0


@pytest.mark.parametrize("prefix,n_valid,n_noise", [
    ("aaaab", 0, 10), ("acacc", 0, 3), ("acccc", 5, 12)])
def test_search_single(prefix, n_valid, n_noise):
    want = _index().search_prefix(prefix)
    assert sum(valid_rule(v, prefix) for v in want) == n_valid
    assert len(want) == n_valid + n_noise
    _check_search([prefix])


def test_search_257_prefixes():
    rng = random.Random(3)
    prefixes = [SyntheticYouTubeClient.generate_random_prefix(rng)
                for _ in range(257)]
    r = _check_search(prefixes)
    # keys of rule-valid slots are distinct per distinct id
    valid = (r["flags"].reshape(-1) & 2) != 0
    ids = [bytes(x) for x in r["ids"].reshape(-1, 11)[valid]]
    keys = r["keys"][valid].tolist()
    assert len(set(zip(ids, keys))) == len(set(ids)) == len(set(keys))


# ---------- first-claim ----------

def _claim_setup(prefixes):
    """Device search results + the Python seen-set's first-occurrence
    mask over the same slots."""
    from crawler_amd.ops import gpu

    idx = _index()
    r = gpu.yt_search(idx, _prefix_tensor(prefixes))
    seen, want = set(), []
    for prefix in prefixes:
        got = idx.search_prefix(prefix)
        for j in range(gpu.YT_SEARCH_SLOTS):
            vid = got[j] if j < len(got) else None
            first = (vid is not None and valid_rule(vid, prefix)
                     and vid not in seen)
            if first:
                seen.add(vid)
            want.append(int(first))
    return r, want


def _repeating_prefixes():
    rng = random.Random(7)
    base = [SyntheticYouTubeClient.generate_random_prefix(rng)
            for _ in range(40)]
    base = [p for p in base
            if any(valid_rule(v, p) for v in _index().search_prefix(p))]
    assert len(base) >= 12
    # repeats inside one call and across calls
    return [base[:8] + base[2:5] + base[:2],
            base[4:12] + base[:3],
            base[10:] + base[6:9] + base[10:]]


def test_first_claim_matches_seen_set_across_calls():
    from crawler_amd.ops import gpu

    calls = _repeating_prefixes()
    flat = [p for c in calls for p in c]
    _, want = _claim_setup(flat)
    assert 0 < sum(want) < sum(
        valid_rule(v, p) for p in flat for v in _index().search_prefix(p))
    table = gpu.YtFirstClaim(DEV, slots_log2=12)
    got, base = [], 0
    for c in calls:
        r = gpu.yt_search(_index(), _prefix_tensor(c))
        valid = (r["flags"].reshape(-1) & 2) != 0
        first = table.claim(r["keys"], valid, base)
        got += first.cpu().tolist()
        base += len(c) * gpu.YT_SEARCH_SLOTS
    assert got == want


def test_first_claim_deterministic_on_fresh_tables():
    from crawler_amd.ops import gpu

    flat = [p for c in _repeating_prefixes() for p in c]
    r, want = _claim_setup(flat)
    valid = (r["flags"].reshape(-1) & 2) != 0
    a = gpu.YtFirstClaim(DEV, slots_log2=12).claim(r["keys"], valid, 0)
    b = gpu.YtFirstClaim(DEV, slots_log2=12).claim(r["keys"], valid, 0)
    assert a.cpu().tolist() == b.cpu().tolist() == want


def _pack_key(vid):
    alph = ("abcdefghijklmnopqrstuvwxyz"
            "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_")
    p = 0
    for ch in vid[:5]:
        p = p * 26 + (ord(ch) - 97)
    k = p << 30
    for i, ch in enumerate(vid[6:]):
        k |= alph.index(ch) << (6 * i)
    return k


def test_keys_stay_distinct():
    """aaaaa-aaaaa, one-character tail differences and tails with '-' and
    '_' all claim separately; the kernel packs keys the same way."""
    from crawler_amd.ops import gpu

    ids = ["aaaaa-aaaaa", "aaaaa-aaaab", "aaaaa-baaaa", "aaaaa-aaaa-",
           "aaaaa-aaaa_", "aaaaa--aaaa", "aaaaa-_aaaa", "aaaab-aaaaa",
           "baaaa-aaaaa", "zzzzz-_____", "aaaaa-aaaaa"]
    keys = [_pack_key(v) for v in ids]
    assert keys[0] == 0 and len(set(keys)) == len(set(ids))
    assert max(keys) < 2 ** 54
    t = gpu.YtFirstClaim(DEV, slots_log2=6)
    first = t.claim(torch.tensor(keys, dtype=torch.int64, device=DEV),
                    None, 0)
    assert first.cpu().tolist() == [1] * 10 + [0]
    # the search kernel's packing for a produced id
    prefix = "acccc"
    r = _search_host([prefix])
    want = _index().search_prefix(prefix)
    for j in range(5):
        assert int(r["keys"][j]) == _pack_key(want[j])


def test_table_grows_and_still_answers():
    from crawler_amd.ops import gpu

    rng = random.Random(1)
    keys = rng.sample(range(1 << 50), 300)
    t = gpu.YtFirstClaim(DEV, slots_log2=6)
    base = 0
    for lo in range(0, 300, 100):
        k = torch.tensor(keys[lo:lo + 100], dtype=torch.int64, device=DEV)
        assert t.claim(k, None, base).cpu().tolist() == [1] * 100
        base += 100
    assert t.grown >= 2 and (1 << t.slots_log2) >= 600
    # every key is remembered across the growth, with its first index
    again = torch.tensor(keys, dtype=torch.int64, device=DEV)
    assert t.claim(again, None, base).cpu().tolist() == [0] * 300
    mask = torch.zeros(300, dtype=torch.uint8, device=DEV)
    mask[::3] = 1
    fresh = torch.tensor([k + (1 << 51) for k in keys], dtype=torch.int64,
                         device=DEV)
    got = t.claim(fresh, mask, base + 300).cpu().tolist()
    assert got == [1 if i % 3 == 0 else 0 for i in range(300)]


def test_full_table_raises():
    """65 distinct keys into a 64-slot table with growth disabled: the
    bounded probe wraps once, sets the error word, and the driver
    raises (the kernel's probe loops run at most `cap` iterations)."""
    from crawler_amd.ops import gpu

    t = gpu.YtFirstClaim(DEV, slots_log2=6, grow=False)
    k = torch.arange(1, 66, dtype=torch.int64, device=DEV)
    with pytest.raises(gpu.YtClaimTableError):
        t.claim(k, None, 0)


# ---------- uploads ----------

@pytest.fixture(scope="module")
def upload_index():
    idx = _index()
    counts = {n: idx.channel(n).video_count for n in (82, 99, 33, 21)}
    assert counts == {82: 0, 99: 29, 33: 10, 21: 11}
    return idx


@pytest.mark.parametrize("limit", [5, 50])
def test_uploads(upload_index, limit):
    from crawler_amd.ops import gpu

    idx = upload_index
    ns = [82, 99, 33, 21] + list(range(100, 357))
    ids, counts = gpu.yt_uploads(
        idx, torch.tensor(ns, dtype=torch.int64, device=DEV), limit)
    torch.cuda.synchronize()
    ids, counts = ids.cpu().numpy(), counts.cpu().tolist()
    assert ids.shape == (len(ns), 29, 11)
    for c, n in enumerate(ns):
        want = idx.channel_uploads(idx.channel_id_of(n), limit)
        assert counts[c] == len(want), n
        got = [bytes(ids[c, k]).decode() for k in range(counts[c])]
        assert got == want, n
        assert not ids[c, counts[c]:].any()


# ---------- id-driven batch builder ----------

def _ids_from_searches(n):
    idx = _index()
    rng = random.Random(2)
    out = []
    while len(out) < n:
        p = SyntheticYouTubeClient.generate_random_prefix(rng)
        out += [v for v in idx.search_prefix(p) if valid_rule(v, p)]
    return out[:n]


def _golden(ids, label):
    idx = _index()
    videos = [idx.video(v) for v in ids]
    pos, rows, channel_of = {}, [], []
    for v in videos:
        if v.channel_id not in pos:
            pos[v.channel_id] = len(rows)
            rows.append(idx.channel(idx.channel_index_of(v.channel_id)))
        channel_of.append(pos[v.channel_id])
    return encode_yt_batch(pack_videos(videos, rows, channel_of, label),
                           now=NOW), len(rows)


@pytest.mark.parametrize("n", [1, 257])
def test_build_batch_from_ids(n):
    from crawler_amd.ops import gpu
    from crawler_amd.youtube.batch import build_batch_from_ids_device

    ids = _ids_from_searches(n)
    golden, k = _golden(ids, "lbl")
    b = build_batch_from_ids_device(_index(), _ids_tensor(ids), DEV,
                                    crawl_label="lbl")
    torch.cuda.synchronize()
    assert b.n == n and b.n_channels == k
    assert encode_yt_batch(b.to("cpu"), now=NOW) == golden
    out, _, _ = gpu.yt_parse_encode(b, now=NOW)
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy()) == b"".join(golden)
