"""The multi-caller / multi-process shapes of the boundary (round-5 review "test gaps"):

  * bench.py under torch.distributed.run with TWO ranks on the ONE GPU of the test box (gloo for the two timing scalars): the real
    GpuBackend, the barriers, the NUMA pinning and the per-rank parity check meet here, not for the first time on the 8-GPU node;
  * PopSift::enqueue called from several caller threads at once (sync_queue.h:24-50: "callable from any caller thread"), next to a
    second PopSift on the same device (two of those are unsafe in the reference: global symbols; allowed here);
  * a 60 s soak of the end-to-end path: the pinned pool and the process RSS stay flat."""
import json
import os
import socket
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from tests.headline_worker import bench_frames
from tests.parity import assert_parity, budget, match_features

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bench(world, extra=()):
    args = ["bench.py", "--gpus", str(world), "--steps", "3", "--warmup", "1", "--full", "--quick", "--no-cpu-baseline", "--no-host-ceiling"] + list(extra)
    if world > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + args
    else:
        cmd = [sys.executable] + args
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4"))
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]                      # rank 0 prints ONE JSON line
    return json.loads(lines[0])


def test_bench_two_ranks_on_one_device():
    """world 2 under torch.distributed.run, both ranks on GPU 0 (--ranks-on-device 0), gloo: one JSON line, n_gpus 2, both ranks'
    parity checks 0 / 0 / 0, and the two ranks together deliver about ONE GPU's rate (they share it)."""
    two = _bench(2, ["--dist-backend", "gloo", "--ranks-on-device", "0"])
    assert two["n_gpus"] == 2 and two["steps"] == 3 and two["warmup"] == 1
    pc = two["parity_checked"]
    assert pc["ranks_checked"] == 2 and pc["frames"] == 8 and pc["keypoints"] > 80000
    assert pc["kp_miss"] == 0 and pc["ori_miss"] == 0 and pc["desc_miss"] == 0 and pc["within_budget"], pc
    one = _bench(1)
    assert one["n_gpus"] == 1 and one["parity_checked"]["kp_miss"] == 0
    ratio = two["value"] / one["value"]
    print("two ranks on one GPU: %.0f Mpix/s, one rank: %.0f Mpix/s, ratio %.3f" % (two["value"], one["value"], ratio))
    # sharing one GPU between two processes costs a little (two sets of worker threads, context switches between the
    # processes' queues); a ratio far from 1 would mean the ranks serialise or the aggregate is computed wrongly
    assert 0.70 < ratio < 1.20, (two["value"], one["value"])


def test_enqueue_from_four_caller_threads_and_a_second_instance(oracle, capi):
    """4 caller threads x 50 enqueue / get on ONE PopSift, a second PopSift on the same device fed by a fifth thread at
    the same time; every result is the oracle's for ITS frame."""
    import bench
    frames = bench_frames(8)
    kw = bench.HEADLINE_KW
    refs = []
    for f in frames:
        r = oracle.run(oracle.default_config(**kw), f)
        refs.append((r.features().copy(), r.descriptors().copy()))
        r.close()
    ps = capi.PopSift(capi.default_config(**kw))
    ps2 = capi.PopSift(capi.default_config(**kw))
    results, errors = [], []
    lock = threading.Lock()

    def caller(tid, obj, n):
        try:
            pending = []
            for j in range(n):
                i = (tid * 3 + j) % len(frames)
                pending.append((i, obj.enqueue(frames[i])))
                if len(pending) >= 4:                            # a few jobs outstanding per caller
                    k, job = pending.pop(0)
                    fb, db = obj.get(job)
                    with lock:
                        results.append((tid, k, fb, db))
            for k, job in pending:
                fb, db = obj.get(job)
                with lock:
                    results.append((tid, k, fb, db))
        except Exception as e:                                   # noqa: BLE001
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=caller, args=(t, ps, 50)) for t in range(4)]
    threads.append(threading.Thread(target=caller, args=(4, ps2, 40)))
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    dt = time.perf_counter() - t0
    assert not errors, errors
    assert all(not t.is_alive() for t in threads)
    ps.close(); ps2.close()
    assert len(results) == 4 * 50 + 40
    tot = dict(kp=0, ori=0, desc=0, n=0)
    for tid, k, fb, db in results:
        fa, da = refs[k]
        assert len(fb) == len(fa) and len(db) == len(da), (tid, k, len(fb), len(fa))
        m = match_features(fa, da, fb, db)
        assert_parity(m, what="caller %d frame %d" % (tid, k), **budget(len(fa)))
        tot["kp"] += m["kp_miss"]; tot["ori"] += m["ori_miss"]; tot["desc"] += m["desc_miss"]; tot["n"] += len(fa)
    b = budget(tot["n"])
    assert tot["kp"] <= b["kp"] and tot["ori"] <= b["ori"] and tot["desc"] <= b["desc"], (tot, b)
    print("5 caller threads, 2 PopSift objects on one device: %d results in %.2f s, %d keypoints checked, misses %s" % (len(results), dt, tot["n"], tot))


def _rss_mb():
    for line in open("/proc/self/status"):
        if line.startswith("VmRSS:"):
            return int(line.split()[1]) / 1024.0
    return 0.0


def test_soak_60s_pinned_pool_and_rss_stay_flat(capi):
    """60 s of the end-to-end path (24 jobs outstanding, results fetched and freed): after the first seconds the pinned pool
    allocates nothing more (every result buffer is a pool hit) and the process RSS does not grow (tools/soak.sh's long
    run as a test; pool / registry leaks were an advisor finding in round 4)."""
    import bench
    from collections import deque
    frames = bench_frames(16)
    ps = capi.PopSift(capi.default_config(**bench.HEADLINE_KW))
    jobs = deque()
    samples = []
    n = 0
    t0 = time.perf_counter()
    next_sample = 5.0
    while True:
        now = time.perf_counter() - t0
        if now >= 60.0:
            break
        if len(jobs) >= 24:
            ps.get_counts(jobs.popleft())
        jobs.append(ps.enqueue(frames[n % len(frames)]))
        n += 1
        if now >= next_sample:
            st = capi.pool_stats(0)
            samples.append((round(now, 1), n, st["allocs"], st["frees"], st["in_use"], st["free_bytes"], round(_rss_mb(), 1)))
            next_sample += 5.0
    while jobs:
        ps.get_counts(jobs.popleft())
    ps.close()
    end = capi.pool_stats(0)
    print("soak: %d frames in 60 s (%.0f frames/s); samples (t, frames, allocs, frees, in_use, free_bytes, rss_mb):" % (n, n / 60.0))
    for s_ in samples:
        print("   ", s_)
    assert n > 60 * 500 and len(samples) >= 10
    first, last = samples[1], samples[-1]                         # from t = 10 s on
    assert last[2] - first[2] <= 4, "the pinned pool kept allocating: %s -> %s" % (first, last)
    early, late = max(x[4] for x in samples[1:6]), max(x[4] for x in samples[6:])
    assert late <= early * 1.10 + (8 << 20), "pinned bytes in use grew: %d -> %d" % (early, late)
    assert last[6] <= first[6] * 1.03 + 32.0, "RSS grew: %.1f -> %.1f MB" % (first[6], last[6])
    print("    after close:", end)
    assert end["in_use"] == 0, end                                # every pinned byte handed back to the pool
