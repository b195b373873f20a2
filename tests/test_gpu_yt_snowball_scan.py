"""csrc/yt_snowball.hip vs its oracles: the channel-id scan against the
BYTES regex (offsets are byte offsets: the str regex disagrees once a
multi-byte character appears), and the channel reverse map against the
index's own ids."""
import random
import re

import numpy as np
import pytest
import torch

from crawler_amd.youtube.batch import _cid_bytes_vec
from crawler_amd.youtube.synth import SyntheticYouTubeIndex

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CID_RE = re.compile(rb"UC[0-9A-Za-z_-]{22}")
CAND_RE = re.compile(rb"(?=UC[0-9A-Za-z_-]{22})")   # every candidate start
CLASS = (b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
         b"abcdefghijklmnopqrstuvwxyz_-")
ID = b"UC" + b"abcdefghijklmnopqrstuv"     # its tail holds no 'U' or 'C'
ID2 = b"UC" + b"0123456789_-zyxwvutsrq"
FILL = b"lorem ipsum, dolor sit amet. "     # no 'U', no 'C', no long run


def filler(n):
    return (FILL * (n // len(FILL) + 1))[:n]


def oracle(texts):
    return [[m.start() for m in CID_RE.finditer(t)] for t in texts]


def scan(texts):
    """Pack back to back, scan on the device; per-text start lists."""
    from crawler_amd.ops import gpu

    blob = b"".join(texts)
    lens = np.array([len(t) for t in texts], dtype=np.int32)
    offs = np.cumsum(lens, dtype=np.int64) - lens
    pool = torch.frombuffer(bytearray(blob or b"\0"),
                            dtype=torch.uint8).to(DEV)
    if not blob:
        pool = pool[:0]
    t_off = torch.from_numpy(offs.astype(np.int64)).to(DEV)
    t_len = torch.from_numpy(lens).to(DEV)
    hit_off, counts = gpu.yt_scan_channel_ids(pool, t_off, t_len)
    assert hit_off.dtype == torch.int64 and counts.dtype == torch.int32
    assert counts.shape == (len(texts),)
    counts = counts.cpu().tolist()
    hits = hit_off.cpu().tolist()
    assert len(hits) == sum(counts)
    out, k = [], 0
    for o, c in zip(offs.tolist(), counts):
        out.append([h - o for h in hits[k:k + c]])
        k += c
    return out


def check(texts):
    want = oracle(texts)
    got = scan(texts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, texts[i])
    return want


# ---------- corpora (CPU-built; their preconditions are asserted) ----------

LENGTHS = [0, 1, 23, 24, 25, 63, 64, 65, 87, 88, 128, 300]


def length_texts():
    out = []
    for n in LENGTHS:
        out.append(filler(n))
        # an id ending exactly at the text's end / a cut-off id
        out.append(filler(n - 24) + ID if n >= 24 else ID[:n])
        # an id at the start
        out.append((ID2 + filler(max(n - 24, 0)))[:n])
        out.append((CLASS * 5)[:n])            # class bytes only, no "UC"
    return out


def sweep_texts():
    out = []
    for start in range(131):
        t = bytearray(filler(200))
        t[start:start + 24] = ID
        out.append(bytes(t))
    return out


def special_texts():
    return [
        b"UCUC" + b"x" * 22,
        ID + ID2,
        ID + CLASS[:30] + ID2,
        b"UC" + b"A" * 100,
        b"UC" * 40,
        b"UC" + b"-_" * 11,
        b"uc" + ID[2:] + b" " + b"Uc" + ID[2:] + b" " + b"uC" + ID[2:],
        ID[:23] + "é".encode() + ID,
        b"UC" + b"a" * 21 + "é".encode() + b"a UC" + b"b" * 21 + b"\xff",
    ]


def neighbour_texts():
    """For every shortfall 1..23: a text that ends that many bytes short
    of a match, then a text that begins with the missing bytes."""
    out = []
    for short in range(1, 24):
        out.append(b"ab " + ID[:24 - short])
        out.append(ID[24 - short:] + b" tail")
    out.append(b"z UC" + b"a" * 21)            # cut off at the pool's end
    return out


def fuzz_texts(seed=20240917, n=2000):
    rng = random.Random(seed)
    seps = [b" ", b".", b"/", b"\n", b"=", b"?"]
    high = ["é".encode(), "—".encode(), b"\xff", b"\x80", "😀".encode()]

    def cls(k):
        return bytes(rng.choice(CLASS) for _ in range(k))

    out = []
    for _ in range(n):
        target = rng.randrange(301)
        t = bytearray()
        while len(t) < target:
            r = rng.random()
            if r < 0.22:
                t += b"UC" + cls(22)
            elif r < 0.34:
                t += b"UC" + cls(rng.randrange(30))
            elif r < 0.44:
                t += b"UC" * rng.randrange(1, 5)
            elif r < 0.50:
                t += rng.choice([b"U", b"C", b"CU", b"UUC"])
            elif r < 0.70:
                t += cls(rng.randrange(1, 30))
            elif r < 0.88:
                t += rng.choice(seps)
            else:
                t += rng.choice(high)
        out.append(bytes(t[:target]))
    return out


# ---------- scan ----------

def test_lengths():
    want = check(length_texts())
    assert any(want) and not all(want)


def test_id_at_every_start_straddles_chunks():
    want = check(sweep_texts())
    assert want == [[s] for s in range(131)]


def test_special_texts():
    want = check(special_texts())
    assert want[0] == [0]
    assert want[1] == [0, 24]
    assert want[2] == [0, 54]
    assert want[3] == [0]
    assert want[4] == [0, 24, 48]
    assert want[5] == [0]
    assert want[6] == []
    assert want[7] == [25]
    assert want[8] == []


def test_neighbour_bytes_never_complete_a_match():
    texts = neighbour_texts()
    # the precondition: scanned as ONE text the pool does match
    assert len(CID_RE.findall(b"".join(texts))) >= 23
    want = check(texts)
    assert want == [[] for _ in texts]


def test_n0_and_n1():
    assert scan([]) == []
    assert check([ID]) == [[0]]
    assert check([b""]) == [[]]


def test_n257_partial_last_block():
    texts = [filler(i % 7) + ID + filler(i % 67) + (ID2 if i % 3 else b"")
             for i in range(257)]
    want = check(texts)
    assert want[256] == [256 % 7] + ([256 % 7 + 24 + 256 % 67]
                                     if 256 % 3 else [])


def test_fuzz():
    texts = fuzz_texts()
    want = oracle(texts)
    # preconditions, tuned on the CPU
    multi = sum(1 for w in want if len(w) >= 2)
    overlap = sum(1 for t, w in zip(texts, want)
                  if len(CAND_RE.findall(t)) > len(w))
    straddle = sum(1 for w in want for s in w if s // 64 != (s + 23) // 64)
    assert multi >= 100 and overlap >= 50 and straddle >= 100
    assert any(len(t) == 0 for t in texts)
    assert any(b"\xff" in t for t in texts)
    got = scan(texts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, texts[i])


def test_text_range_outside_the_pool_is_refused():
    from crawler_amd.ops import gpu

    pool = torch.zeros(100, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 90], dtype=torch.int64, device=DEV)
    for lens in ([10, 11], [-1, 5]):
        with pytest.raises(ValueError, match="outside the pool"):
            gpu.yt_scan_channel_ids(
                pool, off, torch.tensor(lens, dtype=torch.int32,
                                        device=DEV))
    with pytest.raises(ValueError, match="outside the pool"):
        gpu.yt_scan_channel_ids(
            pool, torch.tensor([-1], dtype=torch.int64, device=DEV),
            torch.tensor([5], dtype=torch.int32, device=DEV))


# ---------- reverse map ----------

def _index():
    return SyntheticYouTubeIndex(seed=5, universe_channels=3000)


@pytest.fixture(scope="module")
def all_ids():
    ids = _cid_bytes_vec(_index(), np.arange(3000))
    assert len({bytes(r) for r in ids}) == 3000
    idx = _index()
    for n in (0, 1, 82, 1499, 2999):
        assert bytes(ids[n]).decode() == idx.channel_id_of(n)
    return ids


@pytest.fixture(scope="module")
def rmap():
    from crawler_amd.ops import gpu

    m = gpu.YtChannelReverseMap(_index(), DEV)
    assert m.slots_log2 == 13      # 8192 slots: load <= 0.5
    return m


def _lookup(rmap, rows):
    pool = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).to(DEV)
    off = torch.arange(rows.shape[0], dtype=torch.int64, device=DEV) * 24
    return rmap.lookup(pool, off).cpu().numpy()


def test_every_id_maps_to_its_index(rmap, all_ids):
    got = _lookup(rmap, all_ids)
    assert got.dtype == np.int64
    assert (got == np.arange(3000)).all()
    # in any order, and with unrelated bytes around the ids
    perm = np.random.RandomState(3).permutation(3000)
    padded = np.full((3000, 31), ord("x"), dtype=np.uint8)
    padded[:, 5:29] = all_ids[perm]
    pool = torch.from_numpy(padded.reshape(-1)).to(DEV)
    off = torch.arange(3000, dtype=torch.int64, device=DEV) * 31 + 5
    assert (rmap.lookup(pool, off).cpu().numpy() == perm).all()


def test_mutated_and_absent_ids_map_to_minus_one(rmap, all_ids):
    known = {bytes(r) for r in all_ids}
    mut = all_ids.copy()
    for n in range(3000):
        j = n % 24
        mut[n, j] = ord("V") if mut[n, j] != ord("V") else ord("W")
    assert not any(bytes(r) in known for r in mut)
    assert (_lookup(rmap, mut) == -1).all()
    other = _cid_bytes_vec(
        SyntheticYouTubeIndex(seed=6, universe_channels=3000),
        np.arange(3000))
    beyond = _cid_bytes_vec(_index(), np.arange(3000, 6000))
    rng = np.random.RandomState(9)
    noise = np.frombuffer(CLASS, dtype=np.uint8)[
        rng.randint(0, len(CLASS), size=(3000, 24))]
    zeros = np.zeros((8, 24), dtype=np.uint8)
    for rows in (other, beyond, noise, zeros):
        assert not any(bytes(r) in known for r in rows)
        assert (_lookup(rmap, rows) == -1).all()
    assert rmap.lookup(
        torch.zeros(0, dtype=torch.uint8, device=DEV),
        torch.zeros(0, dtype=torch.int64, device=DEV)).shape == (0,)


def test_table_pinned_too_small_raises(all_ids):
    from crawler_amd.ops import gpu

    with pytest.raises(gpu.YtClaimTableError, match="0x1"):
        gpu.YtChannelReverseMap(_index(), DEV, slots_log2=11)
    # 4096 slots hold 3000 ids (load 0.73): full probing still resolves
    tight = gpu.YtChannelReverseMap(_index(), DEV, slots_log2=12)
    assert (_lookup(tight, all_ids) == np.arange(3000)).all()


def test_lookup_offset_outside_the_pool_is_refused(rmap):
    pool = torch.zeros(40, dtype=torch.uint8, device=DEV)
    for bad in (17, -1):
        with pytest.raises(ValueError, match="outside the pool"):
            rmap.lookup(pool, torch.tensor([0, bad], dtype=torch.int64,
                                           device=DEV))
