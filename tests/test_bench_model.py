"""bench.py's request model of the exact successor search
(dir_search_requests): its host replay of the bucket-directory search
(cx_common.hpp dir_successor) must reach the oracle's successor on every key,
or the requests it counts are not the kernel's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

MAX = (1 << 128) - 1


@pytest.mark.parametrize("kind", ["uniform", "small", "cluster", "edges"])
def test_dir_search_replay_reaches_the_successor(kind):
    import bench
    import oracle as O
    rng = np.random.default_rng(0xD1E)
    if kind == "uniform":
        ids, keys = O.splitmix_keys(11, 1 << 16), O.splitmix_keys(12, 1 << 18)
    elif kind == "small":
        ids, keys = O.splitmix_keys(13, 5), O.splitmix_keys(14, 4000)
    elif kind == "cluster":
        base = 0x0123_4567_89AB << 80
        ids = O.keys_from_ints([base + (int(x) << 30) for x in rng.permutation(5000)] +
                               O.ints_from_keys(O.splitmix_keys(15, 3000)))
        keys = O.keys_from_ints([base + int(x) for x in rng.integers(0, 1 << 44, 20000)] +
                                O.ints_from_keys(O.splitmix_keys(16, 20000)))
    else:
        v = O.ints_from_keys(O.splitmix_keys(17, 3000)) + [0, 1, MAX, MAX - 1]
        ids = O.keys_from_ints(v)
        keys = O.keys_from_ints([(x + d) % (1 << 128) for x in v for d in (-1, 0, 1)] +
                                [0, 1, MAX])
    ring = O.ring_build(ids)
    k = 1
    while (1 << k) < len(ring):
        k += 1
    d, r, ans = bench.dir_search_requests(ring, keys, k + 1, want_index=True)
    assert d == len(keys) and r >= 0
    assert (ans == O.successor(ring, keys)).all()


def test_dump_outputs_whole_batch_and_seeded_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy files of owner / hops / status; a batch
    above the byte budget is cut to one seeded sample of lookups, the same
    lookups in every array and in every run."""
    import torch

    import bench
    q = 5000
    owner = (torch.arange(q, dtype=torch.int64) * 7919 % (1 << 24)).to(torch.int32)
    hops = (torch.arange(q) % 25).to(torch.uint8)
    status = torch.zeros(q, dtype=torch.uint8)
    bench.dump_outputs(str(tmp_path / "all"), 0, 1 << 24, owner, hops, status)
    got = {n: np.load(tmp_path / "all" / f"{n}.npy") for n in ("owner", "hops", "status")}
    assert all(a.dtype == np.float32 and a.shape == (q,) for a in got.values())
    assert (got["owner"] == owner.numpy()).all() and (got["hops"] == hops.numpy()).all()
    assert (got["status"] == 0).all()
    # another rank writes nothing
    bench.dump_outputs(str(tmp_path / "r1"), 1, 1 << 24, owner, hops, status)
    assert not (tmp_path / "r1").exists()
    # a budget of 12 B x 1000 lookups: a sorted sample without repeats, twice the same
    monkeypatch.setattr(bench, "DUMP_BUDGET", 12 * 1000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), 0, 1 << 24, owner, hops, status)
    s1 = {n: np.load(tmp_path / "s1" / f"{n}.npy") for n in got}
    s2 = {n: np.load(tmp_path / "s2" / f"{n}.npy") for n in got}
    assert all(s1[n].shape == (1000,) and (s1[n] == s2[n]).all() for n in got)
    # owner = 7919 i mod 2^24 is injective on i < 5000: recover the sampled lookups
    where = {int(v): i for i, v in enumerate(owner.tolist())}
    idx = np.array([where[int(v)] for v in s1["owner"]])
    assert (np.diff(idx) > 0).all() and (s1["hops"] == hops.numpy()[idx]).all()
    # a ring above 2^24 peers: owner indices need float64
    bench.dump_outputs(str(tmp_path / "big"), 0, 1 << 25, owner, hops, status)
    assert np.load(tmp_path / "big" / "owner.npy").dtype == np.float64


def test_plain_dry_run_is_the_headline_alone():
    """Without --full the run measures no CPU baseline; the line keeps the
    fields later measurements read (CX_BENCH_DRYRUN: no GPU)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(CX_BENCH_DRYRUN="1", CX_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "4", "--warmup", "1"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 4 and rec["warmup"] == 1 and rec["cpu_baseline"] is None
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec
