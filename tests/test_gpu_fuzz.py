"""Seeded fuzz of the HIP parse+encode path vs the CPU oracle.

Generates randomized messages (mixed scripts, escape hazards, random
well-formed entities, random reactions/comments, random t.me material)
through the real packer and asserts byte-identical JSONL + identical
link sets. Deterministic seeds so failures reproduce."""
import datetime as dt
import os

import pytest
import torch

from crawler_amd.ops.golden_batch import encode_batch

from _corpora import fuzz_corpus

pytestmark = pytest.mark.gpu

NOW = dt.datetime(2026, 5, 6, 7, 8, 9, tzinfo=dt.timezone.utc)

_SEEDS = [11, 22, 33]
if os.environ.get("CRAWL_FUZZ_SEEDS"):
    # extended campaigns: CRAWL_FUZZ_SEEDS="1,2,3,..." (evidence runs)
    _SEEDS = [int(x) for x in os.environ["CRAWL_FUZZ_SEEDS"].split(",")]


@pytest.mark.parametrize("seed", _SEEDS)
def test_fuzz_batches_byte_identical(seed):
    from crawler_amd.ops import gpu

    msgs, batch = fuzz_corpus(seed, 300)
    golden_lines, golden_links = encode_batch(batch, now=NOW)
    res = gpu.parse_encode(batch.to("cuda:0"), now=NOW)
    torch.cuda.synchronize()
    out = bytes(res.out.cpu().numpy())
    offs = res.line_off.cpu().numpy()
    lens = res.line_len.cpu().numpy()
    for i, gl in enumerate(golden_lines):
        dev = out[offs[i]: offs[i] + lens[i]]
        assert dev == gl, (
            f"seed {seed} msg {i} "
            f"(type {msgs[i].content_type}):\nGPU: {dev[:300]!r}\n"
            f"CPU: {gl[:300]!r}"
        )
    assert gpu.links_to_python(res) == golden_links
