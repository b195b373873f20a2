"""SeenSet (claim table + bloom) driven with hand-built link hashes.

The end-to-end dedup tests only ever see what the synthetic feed
produces. Here ``link_hash`` / ``link_cnt`` are crafted so the table's
edge behaviour is forced: slots beyond ``cnt`` hold garbage, probe
chains wrap around the end of the table, one launch races on duplicate
hashes, and 0 aliases 1. The oracle is a Python set plus a numpy bloom.
"""
import numpy as np
import pytest
import torch

import _corpora as C

pytestmark = pytest.mark.gpu

MAXL = 8
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def gpu_mod():
    from crawler_amd.ops import gpu

    gpu.require_lib()
    return gpu


def _layout(hashes, cnts, garbage_base=0xBAD0000000000001):
    """Place ``hashes`` row-major into an [n, 8] grid where row i holds
    cnts[i % len(cnts)] valid slots; every slot beyond a row's count
    holds a distinct nonzero garbage hash. Returns (grid uint64[n, 8],
    cnt int32[n], garbage list)."""
    rows, cnt, garbage = [], [], []
    it = iter(hashes)
    left = len(hashes)
    i = 0
    while left:
        c = min(cnts[i % len(cnts)], left)
        row = [next(it) for _ in range(c)]
        left -= c
        while len(row) < MAXL:
            g = (garbage_base + 0x10001 * len(garbage)) & U64
            garbage.append(g)
            row.append(g)
        rows.append(row)
        cnt.append(c)
        i += 1
    return (np.array(rows, dtype=np.uint64),
            np.array(cnt, dtype=np.int32), garbage)


def _result(gpu_mod, grid, cnt):
    """An EncodeResult whose link_hash/link_cnt are ``grid``/``cnt``;
    names are unique per slot with non-zero junk beyond their length."""
    dev = torch.device("cuda:0")
    n = grid.shape[0]
    names = np.full((n, MAXL, 32), 0xEE, dtype=np.uint8)
    lens = np.zeros((n, MAXL), dtype=np.uint8)
    for i in range(n):
        for k in range(MAXL):
            nm = b"name%04d_%d" % (i, k) + b"x" * ((i + k) % 20)
            names[i, k, :len(nm)] = np.frombuffer(nm, dtype=np.uint8)
            lens[i, k] = len(nm)
    t = lambda a: torch.from_numpy(a).to(dev)
    return gpu_mod.EncodeResult(
        out=torch.empty(0, dtype=torch.uint8, device=dev),
        line_off=torch.zeros(n, dtype=torch.int64, device=dev),
        line_len=torch.zeros(n, dtype=torch.int32, device=dev),
        link_name=t(names), link_len=t(lens),
        link_src=torch.zeros((n, MAXL), dtype=torch.uint8, device=dev),
        link_cnt=t(cnt), link_hash=t(grid.view(np.int64)),
    )


def _claim(seen, res):
    mask = seen.claim(res)
    torch.cuda.synchronize()
    return mask.cpu().numpy().astype(bool)


def _table_set(seen):
    tab = seen.table.cpu().numpy().view(np.uint64)
    nz = tab[tab != 0]
    assert len(set(nz.tolist())) == nz.size, "a hash occupies two slots"
    return set(nz.tolist())


def _bloom_oracle(bits_log2, hashes, into=None):
    mask = (1 << bits_log2) - 1
    bloom = (np.zeros((1 << bits_log2) // 32, dtype=np.uint32)
             if into is None else into.copy())
    for h in hashes:
        for b in (h & mask, (h >> 32) & mask):
            bloom[b >> 5] |= np.uint32(1 << (b & 31))
    return bloom


def _valid(grid, cnt):
    return [int(grid[i, k]) for i in range(grid.shape[0])
            for k in range(int(cnt[i]))]


def _remap(h):
    return 1 if h == 0 else h


def test_bloom_bits_exact_and_accumulate(gpu_mod):
    first, second = C.bloom_hashes()
    seen = gpu_mod.SeenSet(torch.device("cuda:0"), slots_log2=10,
                           bloom_bits_log2=10)
    grid, cnt, _ = _layout(first, [3, 0, 8, 1])
    assert sorted(_valid(grid, cnt)) == sorted(first)
    _claim(seen, _result(gpu_mod, grid, cnt))
    want = _bloom_oracle(10, first)
    got = seen.bloom.cpu().numpy().view(np.uint32)
    assert got.shape == want.shape == (32,)
    assert got.tolist() == want.tolist()
    # second round ORs into the first
    grid2, cnt2, _ = _layout(second, [2, 5])
    _claim(seen, _result(gpu_mod, grid2, cnt2))
    want2 = _bloom_oracle(10, second, into=want)
    assert want2.tolist() != want.tolist()
    got2 = seen.bloom.cpu().numpy().view(np.uint32)
    assert got2.tolist() == want2.tolist()


def test_cnt_is_honoured(gpu_mod):
    """Nonzero garbage beyond link_cnt never reaches mask, count, table
    or bloom."""
    valid = C.home_slot_hashes(5, 20, 10, salt=7)
    grid, cnt, garbage = _layout(valid, [3, 0, 8, 1, 5])
    assert garbage and not set(garbage) & set(valid)
    assert (cnt == 0).any() and (cnt == 8).any()
    seen = gpu_mod.SeenSet(torch.device("cuda:0"), slots_log2=10,
                           bloom_bits_log2=10)
    mask = _claim(seen, _result(gpu_mod, grid, cnt))
    want_mask = np.arange(MAXL)[None, :] < cnt[:, None]
    assert (mask == want_mask).all()
    assert seen.new_count() == len(valid)
    assert _table_set(seen) == set(valid)
    got = seen.bloom.cpu().numpy().view(np.uint32)
    assert got.tolist() == _bloom_oracle(10, valid).tolist()


def test_probe_wraps_and_long_chains(gpu_mod):
    last, first = C.wrap_chain_hashes()
    hashes = last + first
    grid, cnt, _ = _layout(hashes, [8])
    seen = gpu_mod.SeenSet(torch.device("cuda:0"), slots_log2=6,
                           bloom_bits_log2=10)
    res = _result(gpu_mod, grid, cnt)
    mask = _claim(seen, res)
    assert mask.sum() == 48 and mask.all()
    assert seen.new_count() == 48
    assert _table_set(seen) == set(hashes)
    # linear probing from slot 63 wraps: one contiguous run 63, 0..46
    tab = seen.table.cpu().numpy().view(np.uint64)
    assert set(np.nonzero(tab)[0].tolist()) == {63} | set(range(47))
    # a second claim finds every hash at the end of its chain
    mask2 = _claim(seen, res)
    assert mask2.sum() == 0
    assert seen.new_count() == 0
    assert _table_set(seen) == set(hashes)


def test_duplicates_inside_one_launch(gpu_mod):
    distinct = C.dup_hashes()
    hashes = [distinct[(j * 7) % 16] for j in range(2048)]
    grid, cnt, _ = _layout(hashes, [8])
    assert grid.shape == (256, 8)
    seen = gpu_mod.SeenSet(torch.device("cuda:0"), slots_log2=10,
                           bloom_bits_log2=10)
    mask = _claim(seen, _result(gpu_mod, grid, cnt))
    assert mask.sum() == 16
    assert seen.new_count() == 16
    winners = grid[mask].tolist()
    assert sorted(winners) == sorted(distinct)   # one winner per hash
    assert _table_set(seen) == set(distinct)


def test_zero_aliases_one(gpu_mod):
    """Hash 0 is stored as 1 (0 marks an empty slot), so 0 and 1 are one
    entry: exactly one of them wins."""
    grid, cnt, _ = _layout([0, 1], [2])
    seen = gpu_mod.SeenSet(torch.device("cuda:0"), slots_log2=6,
                           bloom_bits_log2=10)
    mask = _claim(seen, _result(gpu_mod, grid, cnt))
    assert mask[0, :2].sum() == 1 and mask.sum() == 1
    assert seen.new_count() == 1
    assert _table_set(seen) == {1}


def test_insert_hashes_then_superset_claim(gpu_mod):
    a, b, c, d, e = C.home_slot_hashes(9, 5, 8, salt=50)
    seen = gpu_mod.SeenSet(torch.device("cuda:0"), slots_log2=8,
                           bloom_bits_log2=10)
    pre = np.array([a, b, a, 0, c, b, a], dtype=np.uint64)
    seen.insert_hashes(torch.from_numpy(pre.view(np.int64)).to("cuda:0"))
    torch.cuda.synchronize()
    assert _table_set(seen) == {a, b, c, 1}
    superset = [a, d, b, 0, c, 1, e]
    grid, cnt, _ = _layout(superset, [4, 3])
    mask = _claim(seen, _result(gpu_mod, grid, cnt))
    assert sorted(grid[mask].tolist()) == sorted([d, e])
    assert seen.new_count() == 2
    assert _table_set(seen) == {a, b, c, d, e, 1}


def test_compact_claimed_returns_exactly_the_winners(gpu_mod):
    distinct = C.home_slot_hashes(3, 12, 10, salt=90) + [0]
    hashes = [distinct[(j * 5) % 13] for j in range(60)]
    grid, cnt, garbage = _layout(hashes, [8, 2, 0, 7])
    seen = gpu_mod.SeenSet(torch.device("cuda:0"), slots_log2=10,
                           bloom_bits_log2=10)
    res = _result(gpu_mod, grid, cnt)
    mask_t = seen.claim(res)
    torch.cuda.synchronize()
    mask = mask_t.cpu().numpy().astype(bool)
    assert mask.sum() == 13
    names_c, hashes_c = seen.compact_claimed(res, mask_t)
    assert names_c.shape == (13, 32) and hashes_c.shape == (13,)
    names = res.link_name.cpu().numpy()
    lens = res.link_len.cpu().numpy()
    want = set()
    for i, k in zip(*np.nonzero(mask)):
        nm = bytes(names[i, k, :lens[i, k]])
        want.add((nm + b"\0" * (32 - len(nm)), int(grid[i, k])))
    got_n = names_c.cpu().numpy()
    got_h = hashes_c.cpu().numpy().view(np.uint64)
    got = {(bytes(got_n[j]), int(got_h[j])) for j in range(13)}
    assert got == want
    assert sorted(h for _, h in got) == sorted(distinct)
    assert not {h for _, h in got} & set(garbage)
