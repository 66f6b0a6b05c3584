"""Times zk_poseidon_tree_update and zk_poseidon_tree_append (csrc/poseidon.hip) against what a caller had before them -- one
zk_poseidon_tree_build over the full new leaf array already on the device -- in one process, legs alternated: one JSON line per
measurement.

    python tools/time_poseidon_update.py [--tree-log 20] [--updates 1,64,4096,65536] [--appends 1,4096,65536] [--append-room 65536]
                                         [--reps 7] [--out profiles/poseidon_update.jsonl]

    yardstick    one zk_poseidon_hash_batch call of 2^10 hashes, arity 2: four workgroups, so the latency of ONE hash and with it of one
                 level of an update.  `floor_ms` on every other line is depth x this figure: the dependent chain of hashes from a leaf
                 to the root, which no kernel of one hash per lane gets under.
    update       zk_poseidon_tree_update of `count` distinct drawn leaves of a tree of 2^tree-log drawn leaves at depth tree-log, against
                 zk_poseidon_tree_build over the edited leaf array
    append       zk_poseidon_tree_append of `count` leaves onto a tree built over 2^tree-log - append-room leaves (the first append grows
                 the node buffer: allocation and the device-to-device copy of every level are inside), a second append of the same
                 size where it still fits (the room is there), against zk_poseidon_tree_build over all the leaves

Host clock around each call (every call is complete on return) between device synchronisations.  After one warm-up of each leg the
legs alternate `reps` times; medians with min and max.  `match`: the root after the call equals the root of the rebuilt tree."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zksnark_rs_amd as zk  # noqa: E402


def med(xs):
    return dict(median=round(float(np.median(xs)), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def clocked(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def drawn_elements(torch, count, seed):
    """count x 4 words < r on the device: 60 random bits in the top word keep every element below r"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    a = torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device="cuda", generator=g)
    a[:, 3] &= (1 << 60) - 1
    return a


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree-log", type=int, default=20)
    ap.add_argument("--updates", default="1,64,4096,65536")
    ap.add_argument("--appends", default="1,4096,65536")
    ap.add_argument("--append-room", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = zk.Context(0)
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    depth = args.tree_log
    n_leaves = 1 << depth
    base = dict(tool="time_poseidon_update", depth=depth, reps=args.reps, level_kernel="dense list of changed nodes, wave-aggregated atomicAdd")

    # ---- the yardstick: the latency of one hash ----
    d_in = drawn_elements(torch, 2 << 10, 3).view(1 << 10, 2, 4)
    d_out = torch.zeros((1 << 10, 4), dtype=torch.int64, device="cuda")
    one_hash = lambda: ctx.poseidon_hash_batch(d_in.data_ptr(), 2, 1 << 10, d_out.data_ptr())   # noqa: E731
    clocked(one_hash)
    t_hash = [clocked(one_hash) for _ in range(args.reps)]
    hash_ms = float(np.median(t_hash))
    floor_ms = round(depth * hash_ms, 4)
    emit(dict(base, what="yardstick", call="zk_poseidon_hash_batch, arity 2, 2^10 hashes", match=True, call_ms=med(t_hash), floor_ms=floor_ms))

    d_leaves = drawn_elements(torch, n_leaves, 77)
    built = []

    def build(d, n):
        built.append(ctx.poseidon_tree(d.data_ptr(), depth, n_leaves=n))

    def rebuilt_root(d, n, times):
        """one timed zk_poseidon_tree_build over d[:n]; -> its root"""
        times.append(clocked(lambda: build(d, n)))
        tree = built.pop()
        root = tree.root
        tree.close()
        return root

    # ---- update ----
    tree = ctx.poseidon_tree(d_leaves.data_ptr(), depth, n_leaves=n_leaves)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    for count in [int(s) for s in args.updates.split(",") if s]:
        d_idx = torch.randperm(n_leaves, dtype=torch.int64, device="cuda", generator=g)[:count].contiguous()
        d_val = drawn_elements(torch, count, 100 + count)
        d_leaves[d_idx] = d_val                                                   # the edited leaf array the rebuild starts from
        update = lambda: tree.update_dev(d_idx.data_ptr(), d_val.data_ptr(), count)   # noqa: E731
        t_update, t_build = [], []
        clocked(update)
        match = tree.root == rebuilt_root(d_leaves, n_leaves, [])
        for _ in range(args.reps):                                                # the same leaves and values again: the same work
            t_update.append(clocked(update))
            match = match and tree.root == rebuilt_root(d_leaves, n_leaves, t_build)
        emit(dict(base, what="update", n_leaves=n_leaves, count=count, match=bool(match), update_ms=med(t_update), rebuild_ms=med(t_build),
                  rebuild_over_update=round(float(np.median(t_build)) / float(np.median(t_update)), 3), floor_ms=floor_ms))
    tree.close()

    # ---- append ----
    n_base = n_leaves - args.append_room
    for count in [int(s) for s in args.appends.split(",") if s]:
        again = n_base + 2 * count <= n_leaves
        t_append, t_again, t_build = [], [], []
        match = True
        for rep in range(args.reps + 1):                                          # the first round is the warm-up
            build(d_leaves, n_base)
            grown = built.pop()
            ta = clocked(lambda: grown.append_dev(d_leaves.data_ptr() + 32 * n_base, count))
            root = grown.root
            tb = clocked(lambda: grown.append_dev(d_leaves.data_ptr() + 32 * (n_base + count), count)) if again else None
            root_again = grown.root
            n_after = grown.n_leaves
            grown.close()
            times = []
            match = match and root == rebuilt_root(d_leaves, n_base + count, times)
            if again:
                match = match and root_again == rebuilt_root(d_leaves, n_base + 2 * count, []) and n_after == n_base + 2 * count
            if rep:
                t_append.append(ta)
                t_build += times
                if again:
                    t_again.append(tb)
        emit(dict(base, what="append", n_leaves=n_base, count=count, match=bool(match), append_ms=med(t_append),
                  append_again_ms=med(t_again) if again else None, rebuild_ms=med(t_build),
                  rebuild_over_append=round(float(np.median(t_build)) / float(np.median(t_append)), 3), floor_ms=floor_ms))
    if out:
        out.close()


if __name__ == "__main__":
    main()
