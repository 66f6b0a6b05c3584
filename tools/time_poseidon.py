"""Times Poseidon on the device (csrc/poseidon.hip) and the membership circuit it feeds, in one process, legs alternated: one JSON line
per measurement.

    python tools/time_poseidon.py [--hashes 10,16,20,24] [--tree-log 20] [--paths 4096] [--counts 64,4096,65536] [--prove 4096]
                                  [--reps 5] [--out profiles/poseidon.jsonl]

    hash_batch   zk_poseidon_hash_batch, arity 2, on 2^k drawn input pairs resident on the device: host clock around the call (complete
                 on return) and the k_poseidon launch alone (device events, option "profile" = 2, in runs of their own), next to
                 single-thread zk_poseidon_hash on the host over the first `--host-sample` of the same inputs.  The kernel does 828
                 field multiplications per hash (243 in the S-boxes, 585 in the mix); `mults_of_yardstick` is its time per hash over
                 828 multiplications at the rate of the yardstick: the forward NTT of 2^22 elements (zk_ntt_fr, device events over its
                 kernels, 2^21 x 22 butterfly multiplications), measured in the same run.  The NTT streams its data through HBM once per
                 pass, the hash keeps its state in registers: the figure compares rates, not kernels of one kind.
    tree         zk_poseidon_tree_build over 2^tree-log drawn leaves at depth tree-log, and zk_poseidon_tree_paths for `--paths` drawn
                 indices, host clock around each call
    membership   the depth-`tree-log` membership circuit (zk_builder_merkle_root; public: the root) over that tree: zk_mixgen_run fed by
                 zk_poseidon_tree_paths' outputs against zk_witgen_run on the same inputs, and paths -> zk_mixgen_run ->
                 zk_prove_batch_submit in batches of 64, two batches in flight, as proofs per second

After one warm-up of each leg the legs alternate `reps` times; medians with min and max.  `match`: the device digests equal the host's
on the sample, the root equals the fold of a path on the host, both witness paths agree word for word on the first 64 instances and
the first batch of proofs verifies against the tree's root."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd import poseidon  # noqa: E402
from zksnark_rs_amd.circuit import Builder, Mixgen, Witgen  # noqa: E402

MULS_SBOX, MULS_MIX = 3 * (8 * 3 + 57), 9 * (8 + 57)       # arity 2: 243 + 585 = 828


def med(xs):
    return dict(median=round(float(np.median(xs)), 4), min=round(min(xs), 4), max=round(max(xs), 4))


def clocked(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def profiled(ctx, fn, prefix):
    """device-event time of the launches whose name starts with `prefix` during fn(), ms, and their names"""
    ctx.set_option("profile", 2)
    ctx.profile_reset()
    fn()
    prof = ctx.profile()
    ctx.set_option("profile", 0)
    hit = {k: v for k, v in prof.items() if k.startswith(prefix)}
    return sum(v["total_ms"] for v in hit.values()), sorted(hit)


def drawn_elements(torch, count, seed):
    """count x 4 words < r on the device: 62 random bits in the top word keep every element below r"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    a = torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device="cuda", generator=g)
    a[:, 3] &= (1 << 60) - 1
    return a


def membership_circuit(depth):
    b = Builder()
    leaf = b.new_wire()
    sibs = [b.new_wire() for _ in range(depth)]
    dirs = b.new_bits(depth)
    return b.finish([b.merkle_root(leaf, sibs, dirs)])


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--hashes", default="10,16,20,24")
    ap.add_argument("--host-sample", type=int, default=2048)
    ap.add_argument("--ntt-log", type=int, default=22)
    ap.add_argument("--tree-log", type=int, default=20)
    ap.add_argument("--paths", type=int, default=4096)
    ap.add_argument("--counts", default="64,4096,65536")
    ap.add_argument("--prove", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = zk.Context(0)
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    # ---- the yardstick: the forward NTT's butterfly multiplications ----
    n = 1 << args.ntt_log
    host = drawn_elements(torch, n, 1).cpu().numpy().view(np.uint64)
    ctx.ntt_fr(host)                                                               # warm-up: tables, code objects
    ntt_ms, ntt_names = [], []
    for _ in range(args.reps):
        ms, ntt_names = profiled(ctx, lambda: ctx.ntt_fr(host), "ntt")
        ntt_ms.append(ms)
    ntt_muls = (n // 2) * args.ntt_log
    ns_per_mul = float(np.median(ntt_ms)) * 1e6 / ntt_muls
    emit(dict(tool="time_poseidon", what="yardstick", kernel="zk_ntt_fr forward, 2^%d elements" % args.ntt_log, launches=ntt_names,
              kernels_ms=med(ntt_ms), butterfly_multiplications=ntt_muls, ns_per_multiplication=round(ns_per_mul, 6), reps=args.reps))

    # ---- hash_batch ----
    for log_count in [int(s) for s in args.hashes.split(",") if s]:
        count = 1 << log_count
        d_in = drawn_elements(torch, 2 * count, 2 + log_count).view(count, 2, 4)
        d_out = torch.zeros((count, 4), dtype=torch.int64, device="cuda")
        call = lambda: ctx.poseidon_hash_batch(d_in.data_ptr(), 2, count, d_out.data_ptr())   # noqa: E731
        sample = min(count, args.host_sample)
        rows = [zk.limbs_to_ints(r) for r in d_in[:sample].cpu().numpy().view(np.uint64)]
        clocked(call)
        t0 = time.perf_counter()
        want = [poseidon.hash(r) for r in rows]
        host_ns = (time.perf_counter() - t0) * 1e9 / sample       # through ctypes: the binding's per-call cost is inside
        match = zk.limbs_to_ints(d_out[:sample].cpu().numpy().view(np.uint64)) == want
        profiled(ctx, call, "poseidon")
        t_call, t_kernel = [], []
        for _ in range(args.reps):
            t_call.append(clocked(call))
            t_kernel.append(profiled(ctx, call, "poseidon")[0])
        call_ms, kernel_ms = float(np.median(t_call)), float(np.median(t_kernel))
        kernel_ns = kernel_ms * 1e6 / count
        emit(dict(tool="time_poseidon", what="hash_batch", arity=2, count=count, reps=args.reps, match=bool(match), call_ms=med(t_call),
                  kernel_ms=med(t_kernel), hashes_per_s=round(count / call_ms * 1e3, 1), ns_per_hash_call=round(call_ms * 1e6 / count, 3),
                  kernel_hashes_per_s=round(count / kernel_ms * 1e3, 1), ns_per_hash_kernel=round(kernel_ns, 3),
                  host_single_thread_ns_per_hash=round(host_ns, 1), host_sample=sample, host_over_kernel=round(host_ns / kernel_ns, 1),
                  multiplications_per_hash=MULS_SBOX + MULS_MIX, mix_share_of_multiplications=round(MULS_MIX / (MULS_SBOX + MULS_MIX), 4),
                  ns_per_multiplication_kernel=round(kernel_ns / (MULS_SBOX + MULS_MIX), 6),
                  mults_of_yardstick=round(kernel_ns / ((MULS_SBOX + MULS_MIX) * ns_per_mul), 3)))
        del d_in, d_out
        torch.cuda.empty_cache()

    # ---- the tree and its paths ----
    depth = args.tree_log
    n_leaves = 1 << depth
    d_leaves = drawn_elements(torch, n_leaves, 77)
    trees = []
    build = lambda: trees.append(ctx.poseidon_tree(d_leaves.data_ptr(), depth, n_leaves=n_leaves))   # noqa: E731
    clocked(build)
    t_build = []
    for _ in range(args.reps):
        trees.pop().close()
        t_build.append(clocked(build))
    tree = trees[0]
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    most = max([args.paths, args.prove] + [int(s) for s in args.counts.split(",") if s])
    d_idx = torch.randint(0, n_leaves, (most,), dtype=torch.int64, device="cuda", generator=g)
    d_f = torch.zeros((most, depth + 1, 4), dtype=torch.int64, device="cuda")
    d_b = torch.zeros((most, tree.bit_bytes), dtype=torch.uint8, device="cuda")
    paths = lambda count: tree.paths_dev(d_idx.data_ptr(), count, d_f.data_ptr(), d_b.data_ptr())   # noqa: E731
    clocked(lambda: paths(args.paths))
    t_paths = [clocked(lambda: paths(args.paths)) for _ in range(args.reps)]
    f0, b0 = d_f[0].cpu().numpy().view(np.uint64), bytes(d_b[0].cpu().numpy())
    cur, index = zk.limbs_to_int(f0[0]), int.from_bytes(b0, "little")
    for k in range(depth):
        sib = zk.limbs_to_int(f0[1 + k])
        cur = poseidon.hash([sib, cur] if (index >> k) & 1 else [cur, sib])
    build_ms = float(np.median(t_build))
    emit(dict(tool="time_poseidon", what="tree", n_leaves=n_leaves, depth=depth, reps=args.reps, match=bool(cur == tree.root and index == int(d_idx[0])),
              build_ms=med(t_build), hashes=n_leaves - 1, build_hashes_per_s=round((n_leaves - 1) / build_ms * 1e3, 1), launches=depth,
              paths=args.paths, paths_ms=med(t_paths), paths_per_s=round(args.paths / float(np.median(t_paths)) * 1e3, 1)))

    # ---- the membership circuit ----
    c = membership_circuit(depth)
    dims = c.mixed_dims()
    mg, wg = Mixgen(ctx, c), Witgen(ctx, c)
    paths(most)
    d_tape = torch.zeros((most, 2 * depth + 1, 4), dtype=torch.int64, device="cuda")       # the same inputs in creation order
    d_tape[:, :depth + 1] = d_f
    for k in range(depth):
        d_tape[:, depth + 1 + k, 0] = (d_idx >> k) & 1
    base = dict(tool="time_poseidon", what="membership", depth=depth, m=c.m, n=c.n, reps=args.reps, **dims)
    for count in [int(s) for s in args.counts.split(",") if s]:
        d_w = torch.empty((count, c.m, 4), dtype=torch.int64, device="cuda")
        legs = {"mixgen": lambda: mg.run(d_b.data_ptr(), d_f.data_ptr(), count, d_w.data_ptr()),
                "witgen": lambda: wg.run(d_tape.data_ptr(), count, d_w.data_ptr())}
        first = {}
        for name, call in legs.items():
            d_w.zero_()
            clocked(call)
            first[name] = d_w[:min(count, 64)].cpu().numpy()
        match = bool(np.array_equal(first["mixgen"], first["witgen"])) and zk.limbs_to_int(first["mixgen"][0, 1].view(np.uint64)) == tree.root
        t = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, call in legs.items():
                t[name].append(clocked(call))
        mix, tape = float(np.median(t["mixgen"])), float(np.median(t["witgen"]))
        emit(dict(base, count=count, match=match, mixgen_ms=med(t["mixgen"]), witgen_ms=med(t["witgen"]), witgen_over_mixgen=round(tape / mix, 3),
                  mixgen_witnesses_per_s=round(count / mix * 1e3, 1), witgen_witnesses_per_s=round(count / tape * 1e3, 1)))
        del d_w
        torch.cuda.empty_cache()

    count = args.prove
    qap = c.qap_sparse_unity(ctx)
    rng = zk.SplitMix64(11)
    crs = ctx.setup(qap, zk.ints_to_limbs([rng.fr() for _ in range(5)]))
    d_w = torch.empty((count, c.m, 4), dtype=torch.int64, device="cuda")
    rs = [rng.fr() for _ in range(64)]
    kept = []

    def generate_and_prove():
        paths(count)
        mg.run(d_b.data_ptr(), d_f.data_ptr(), count, d_w.data_ptr())
        tickets, proofs = [], []
        for first in range(0, count, 64):
            nb = min(64, count - first)
            ptrs = [d_w.data_ptr() + (first + j) * c.m * 32 for j in range(nb)]
            tickets.append((ctx.prove_batch_submit(crs, qap, ptrs, [c.m] * nb, rs[:nb], rs[:nb]), nb))
            if len(tickets) == 2:
                proofs += ctx.prove_batch_wait(*tickets.pop(0))
        for tk in tickets:
            proofs += ctx.prove_batch_wait(*tk)
        kept[:] = proofs[:64]

    clocked(generate_and_prove)
    public = np.tile(zk.ints_to_limbs([tree.root]).reshape(1, 1, 4), (len(kept), 1, 1))
    match = bool(ctx.verify_batch(crs, public, kept).all())
    t_prove = [clocked(generate_and_prove) for _ in range(args.reps)]
    emit(dict(base, what="membership_prove", count=count, match=match, qap_n=qap.n, batch=64, in_flight=2, generate_and_prove_ms=med(t_prove),
              proofs_per_s=round(count / float(np.median(t_prove)) * 1e3, 1)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
