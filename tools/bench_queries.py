#!/usr/bin/env python3
"""Measures the batched InterestedIn queries (gw_nearest, gw_neighbors_batch)
on the config #3 population (1M clustered entities) against the
two baselines the library already had:

  (a) gw_total_neighbors: k_count_all, the same window walk over every present
      entity with no filter, no gather and no output -- the floor for the walk;
  (b) a loop of gw_neighbors over 1,000 of the same slots (one blocking call
      per slot), wall time per slot.

Query slots are device-resident (GW_QUERY_SLOTS_ON_DEVICE), outputs stay on the
device.  Times: the calls' device_us (HIP events around the device work) and
the host's wall clock around each call (every call ends in a stream
synchronise); medians over --reps calls after --warmup calls.  Writes one JSON
object (default profiles/queries_bench.json) and prints it.

    python tools/bench_queries.py [--entities 1000000] [--reps 9]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from goworld_amd import gpuaoi, traces  # noqa: E402


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def timed(fn, warmup, reps):
    """fn() -> device_us or None; (median device_us, median wall us, last result)."""
    dev, wall, r = [], [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        if i >= warmup:
            wall.append((t1 - t0) * 1e6)
            dev.append(r.device_us if hasattr(r, "device_us") else np.nan)
    return med(dev), med(wall), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--side", type=float, default=32768.0)
    ap.add_argument("--sample", type=int, default=100_000)
    ap.add_argument("--loop-slots", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queries_bench.json"))
    a = ap.parse_args()

    tr = traces.config3(ticks=1, seed=3, n=a.entities, side=a.side)
    g = gpuaoi.GpuAOI(a.device)
    sid, base = gpuaoi.load_space(g, tr, chunk=1 << 18)
    g.sync_collect(copy=False)
    g.submit(traces.with_global_slots(tr.ticks[0], base))
    g.tick(copy=False)                                  # the state of a flush, as game logic sees it
    g.sync_collect(copy=False)

    rng = np.random.default_rng(3)
    n = tr.capacity
    every = np.arange(n, dtype=np.uint32) + np.uint32(base)     # config #3: every slot is present
    # three entity classes in the low byte and an "alive" bit: Monster.AI's TypeName and hp tests
    tags = (rng.integers(0, 3, n) | (rng.integers(0, 2, n) << 8)).astype(np.uint32)
    g.set_tags(every, tags)
    sample = np.sort(rng.choice(every, min(a.sample, n), replace=False)).astype(np.uint32)
    d_every, d_sample = g.dev_alloc(every.nbytes), g.dev_alloc(sample.nbytes)
    g.h2d(d_every, every)
    g.h2d(d_sample, sample)

    res = {"bench": "queries", "entities": n, "side": a.side, "aoi_dist": tr.d, "reps": a.reps,
           "sample": len(sample)}
    total = g.total_neighbors()
    res["total_neighbors"] = total
    _, wall_a, _ = timed(lambda: g.total_neighbors(), a.warmup, a.reps)
    res["a_total_neighbors_wall_us"] = wall_a

    cases = (("all", d_every, n), ("sample", d_sample, len(sample)))
    # everyone; one class with its alive bit (a sixth of the entities); and two filters nobody
    # passes, which split gw_nearest's cost: "walk_only" (mask 0, value 1) is decided without
    # reading a tag, so it is the window walk alone; "tags_only" reads the tag of every related
    # entity but gathers no position
    filters = (("everyone", 0, 0), ("class1_alive", 0x1FF, 0x101), ("walk_only", 0, 1),
               ("tags_only", 0xFFFFFFFF, 0xDEAD0000))
    for cname, dptr, cnt in cases:
        for fname, mask, value in filters:
            key = f"{cname}_{fname}"
            dev, wall, o = timed(lambda: g.nearest_raw(dptr, mask, value, copy=False, n=cnt), a.warmup, a.reps)
            res[f"nearest_{key}"] = {"device_us": dev, "wall_us": wall, "queries": cnt, "bytes_alg": o.bytes_alg,
                                     "GBps_alg": o.bytes_alg / dev / 1e3 if dev else None,
                                     "us_per_query": dev / cnt}
            dev, wall, o = timed(lambda: g.neighbors_batch_raw(dptr, mask, value, copy=False, n=cnt), a.warmup,
                                 a.reps)
            res[f"lists_{key}"] = {"device_us": dev, "wall_us": wall, "queries": cnt, "entries": o.n_nbr,
                                   "bytes_alg": o.bytes_alg, "GBps_alg": o.bytes_alg / dev / 1e3 if dev else None,
                                   "us_per_query": dev / cnt}
    assert res["lists_all_everyone"]["entries"] == total       # the same sets as the old count

    # (b) one blocking gw_neighbors call per slot
    loop = sample[:: max(1, len(sample) // a.loop_slots)][: a.loop_slots]
    import ctypes as C
    buf = np.zeros(1 << 20, np.uint32)                  # one call per slot fills it (no count-then-fill pair)
    cnt_out = C.c_uint32()

    def one(s):
        rc = gpuaoi.lib().gw_neighbors(g._h, int(s), buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(cnt_out))
        assert rc == 0
        return cnt_out.value
    for s in loop[:20]:
        one(s)
    t0 = time.perf_counter()
    got = 0
    for s in loop:
        got += one(s)
    t1 = time.perf_counter()
    res["b_neighbors_loop"] = {"slots": len(loop), "entries": got, "wall_us_per_slot": (t1 - t0) * 1e6 / len(loop)}

    near_all = res["nearest_all_everyone"]
    res["ratio_nearest_all_to_a"] = near_all["wall_us"] / wall_a
    res["ratio_nearest_all_device_to_a_wall"] = near_all["device_us"] / wall_a
    res["ratio_lists_all_to_a"] = res["lists_all_everyone"]["wall_us"] / wall_a
    walk = res["nearest_all_walk_only"]["device_us"]
    res["nearest_all_device_us_split"] = {
        "walk": walk,
        # "everyone" matches without reading a tag: its cost over the walk is the gather of the
        # matching entities' 64-B lines and the running minimum
        "position_gather_and_min": near_all["device_us"] - walk,
        # what reading the tag of every related entity adds to the walk (no position read)
        "tag_gather": res["nearest_all_tags_only"]["device_us"] - walk}
    res["ratio_nearest_all_to_walk_only"] = near_all["device_us"] / walk
    per_b = res["b_neighbors_loop"]["wall_us_per_slot"]
    res["per_query_speedup_nearest_vs_b"] = per_b / (res["nearest_sample_everyone"]["wall_us"] / len(sample))
    res["per_query_speedup_lists_vs_b"] = per_b / (res["lists_sample_everyone"]["wall_us"] / len(sample))
    g.dev_free(d_every)
    g.dev_free(d_sample)
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
