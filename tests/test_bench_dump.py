"""bench.py --dump-outputs: the files hold what the last timed step
produced, in float32/float64, sampled with a fixed seed when large."""
import datetime as dt
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench

NAMES = ["jsonl_block_sums", "jsonl_sample", "line_off", "line_len",
         "link_cnt", "link_hash", "new_discoveries"]


def _load(d):
    return {n: np.load(os.path.join(str(d), n + ".npy")) for n in NAMES}


def _fake_last(n=300, nbytes=5000, seed=3):
    g = torch.Generator().manual_seed(seed)
    line_len = torch.randint(1, 40, (n,), generator=g, dtype=torch.int32)
    line_off = torch.zeros(n, dtype=torch.int64)
    line_off[1:] = torch.cumsum(line_len.to(torch.int64)[:-1], 0)
    return dict(
        jsonl=torch.randint(0, 256, (nbytes,), generator=g,
                            dtype=torch.uint8),
        line_off=line_off, line_len=line_len,
        link_cnt=torch.randint(0, 9, (n,), generator=g, dtype=torch.int32),
        link_hash=torch.randint(-2**63, 2**63 - 1, (n, 8), generator=g,
                                dtype=torch.int64),
        new_discoveries=17,
    )


def test_dump_small_output_is_written_whole(tmp_path):
    last = _fake_last()
    bench.dump_outputs(str(tmp_path), last)
    got = _load(tmp_path)
    for name, arr in got.items():
        assert arr.dtype in (np.float32, np.float64), name
    raw = last["jsonl"].numpy()
    assert np.array_equal(got["jsonl_sample"], raw.astype(np.float32))
    assert got["jsonl_block_sums"].tolist() == [float(raw.sum())]
    assert np.array_equal(got["line_off"], last["line_off"].numpy())
    assert np.array_equal(got["line_len"], last["line_len"].numpy())
    assert np.array_equal(got["link_cnt"], last["link_cnt"].numpy())
    h = last["link_hash"].numpy().view(np.uint64)
    hi, lo = got["link_hash"][..., 0], got["link_hash"][..., 1]
    back = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    assert np.array_equal(back, h)
    assert got["new_discoveries"].tolist() == [17.0]


def test_dump_large_output_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 100)
    monkeypatch.setattr(bench, "DUMP_HASH_ROWS", 10)
    monkeypatch.setattr(bench, "DUMP_WINDOWS", 4)
    monkeypatch.setattr(bench, "DUMP_WINDOW", 64)
    monkeypatch.setattr(bench, "DUMP_BLOCK", 1024)
    last = _fake_last()
    bench.dump_outputs(str(tmp_path / "a"), last)
    bench.dump_outputs(str(tmp_path / "b"), _fake_last())
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), name
    assert a["jsonl_sample"].shape == (4 * 64,)
    assert a["line_off"].shape == a["line_len"].shape == (100,)
    assert a["link_cnt"].shape == (100,)
    assert a["link_hash"].shape == (10, 8, 2)
    raw = last["jsonl"].numpy().astype(np.float64)
    sums = a["jsonl_block_sums"]
    assert sums.shape == (5,)  # 4 whole 1024-byte blocks + the tail
    assert sums[:4].tolist() == raw[:4096].reshape(4, 1024).sum(1).tolist()
    assert sums[4] == raw[4096:].sum()
    # the sampled rows are rows of the full arrays, in order
    off = last["line_off"].numpy()
    assert np.all(np.diff(a["line_off"]) > 0)
    assert np.isin(a["line_off"], off).all()
    # a different output at the same sizes is sampled at the same places
    other = _fake_last(seed=4)
    bench.dump_outputs(str(tmp_path / "c"), other)
    c = _load(tmp_path / "c")
    assert not np.array_equal(a["jsonl_sample"], c["jsonl_sample"])
    rows = np.flatnonzero(np.isin(off, a["line_off"]))
    assert np.array_equal(c["line_len"],
                          other["line_len"].numpy()[rows])


@pytest.mark.gpu
def test_bench_dump_matches_golden_last_step(tmp_path, monkeypatch, capsys):
    """A tiny plain run: the dumped JSONL is the golden encoding of the
    chunk the last timed step processed, and --steps is the number of
    timed steps."""
    from crawler_amd.feed import FeedConfig, SyntheticFeed
    from crawler_amd.ops.golden_batch import encode_batch

    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
        "--channels", "4", "--posts", "64", "--chunk-channels", "2",
        "--dump-outputs", str(tmp_path)])
    bench.main()
    line = [l for l in capsys.readouterr().out.splitlines()
            if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["config"]["p50_channel_latency_ms"] is None
    assert res["config"]["gpu_busy_sampled"] is None

    # steps 0..2 cycle chunks 0,1,0: the last timed step saw channels 0,1
    feed = SyntheticFeed(FeedConfig(seed=1234, universe=1_000_000,
                                    comment_rate=0.02,
                                    max_comments_per_post=3))
    batch = feed.build_batch(np.arange(2), posts_per_channel=64)
    now = dt.datetime(2026, 1, 1, tzinfo=dt.timezone.utc)
    lines, links = encode_batch(batch, now=now)
    expect = np.frombuffer(b"".join(lines), dtype=np.uint8)
    got = _load(tmp_path)
    assert np.array_equal(got["jsonl_sample"], expect.astype(np.float32))
    assert got["jsonl_block_sums"].sum() == float(expect.sum())
    assert got["line_len"].tolist() == [float(len(l)) for l in lines]
    assert got["link_cnt"].tolist() == [float(len(l)) for l in links]
    assert got["link_hash"].shape == (128, 8, 2)
