"""Times Baby Jubjub on the device (csrc/babyjub.hip) in one process, legs alternated: one JSON line per measurement.

    python tools/time_babyjub.py [--logs 10,16,20] [--chain-log 20] [--host-sample 256] [--reps 5] [--out profiles/babyjub.jsonl]

    mul_batch    zk_babyjub_mul_batch, fixed base and variable base, on 2^k drawn 256-bit scalars (and drawn multiples of Generator)
                 resident on the device, next to the yardstick zk_poseidon_hash_batch of arity 2 at the same count.  The three legs
                 alternate `reps` times after one warm-up each: host clock around the call (complete on return) and the kernel alone
                 (device events, option "profile" = 2, in runs of their own).  Single-thread zk_babyjub_mul on the host over the first
                 `--host-sample` scalars.  `of_yardstick`: the kernel's time per point over (its field multiplications per point) x
                 (the hash kernel's time per multiplication at that count, 828 multiplications a hash).
    chain        secrets -> keys (mul_batch, fixed base) -> leaves (poseidon_hash_batch, arity 2, on the packed keys as they lie) ->
                 zk_poseidon_tree_build at 2^chain-log, end to end, host clock

`match`: the device results equal the host's on the sample; the chain's root equals the root of a tree built from the leaves alone."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd import babyjub  # noqa: E402

MULS_HASH = 828                                             # arity 2: 243 in the S-boxes, 585 in the mix
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MULS_INV = 256 + bin(R - 2).count("1") + 2                  # x^(r - 2) over 256 exponent bits: a squaring a bit, a multiplication per set bit; X Zinv, Y Zinv
MULS_FIXED = (256 // babyjub.FIXED_WINDOW - 1) * 12 + MULS_INV + 2                       # 63 mixed additions, the inversion, to_canonical twice
MULS_VAR = (256 // babyjub.VAR_WINDOW) * (2 * 8 + 13) + 8 + 12 + 2 + MULS_INV + 2        # per window two doublings and an addition; 2 P, 3 P; loads


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
    """device-event time of the launches whose name starts with `prefix` during fn(), ms"""
    ctx.set_option("profile", 2)
    ctx.profile_reset()
    fn()
    prof = ctx.profile()
    ctx.set_option("profile", 0)
    return sum(v["total_ms"] for k, v in prof.items() if k.startswith(prefix))


def drawn_words(torch, count, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device="cuda", generator=g)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="10,16,20")
    ap.add_argument("--chain-log", type=int, default=20)
    ap.add_argument("--host-sample", type=int, default=256)
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

    for log_count in [int(s) for s in args.logs.split(",") if s]:
        count = 1 << log_count
        d_s = drawn_words(torch, count, 10 + log_count)
        d_small = drawn_words(torch, count, 40 + log_count)
        d_small[:, 1:] = 0
        d_p = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
        d_fixed = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
        d_var = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
        d_hash = torch.zeros((count, 4), dtype=torch.int64, device="cuda")
        # the variable base's points: drawn multiples of Generator, made on the device by the kernel under test from a host point
        gen = np.tile(zk.ints_to_limbs(list(babyjub.params()["generator"])).reshape(1, 8), (count, 1))
        d_gen = torch.from_numpy(gen.view(np.int64)).to("cuda")
        torch.cuda.synchronize()
        ctx.babyjub_mul_batch(d_small.data_ptr(), d_gen.data_ptr(), count, d_p.data_ptr(), 0)
        legs = {"fixed": (lambda: ctx.babyjub_mul_batch(d_s.data_ptr(), None, count, d_fixed.data_ptr(), 0), "babyjub_mul_fixed"),
                "var": (lambda: ctx.babyjub_mul_batch(d_s.data_ptr(), d_p.data_ptr(), count, d_var.data_ptr(), 0), "babyjub_mul_var"),
                "hash": (lambda: ctx.poseidon_hash_batch(d_p.data_ptr(), 2, count, d_hash.data_ptr()), "poseidon")}
        for call, prefix in legs.values():
            clocked(call)
            profiled(ctx, call, prefix)
        t_call, t_kernel = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(args.reps):
            for name, (call, prefix) in legs.items():
                t_call[name].append(clocked(call))
                t_kernel[name].append(profiled(ctx, call, prefix))
        sample = min(count, args.host_sample)
        ks = [int(x) for x in zk.limbs_to_ints(d_s[:sample].cpu().numpy().view(np.uint64))]
        pts = [tuple(zk.limbs_to_ints(p)) for p in d_p[:sample].cpu().numpy().view(np.uint64).reshape(sample, 2, 4)]
        t0 = time.perf_counter()
        want_fixed = [babyjub.mul(k) for k in ks]
        host_ns = (time.perf_counter() - t0) * 1e9 / sample       # through ctypes: the binding's per-call cost is inside
        want_var = [babyjub.mul(k, p) for k, p in zip(ks, pts)]
        got_fixed = [tuple(zk.limbs_to_ints(p)) for p in d_fixed[:sample].cpu().numpy().view(np.uint64).reshape(sample, 2, 4)]
        got_var = [tuple(zk.limbs_to_ints(p)) for p in d_var[:sample].cpu().numpy().view(np.uint64).reshape(sample, 2, 4)]
        hash_ns_per_mul = float(np.median(t_kernel["hash"])) * 1e6 / count / MULS_HASH
        line = dict(tool="time_babyjub", what="mul_batch", count=count, reps=args.reps, match=bool(got_fixed == want_fixed and got_var == want_var),
                    host_single_thread_ns_per_mul_fixed=round(host_ns, 1), host_sample=sample,
                    hash_call_ms=med(t_call["hash"]), hash_kernel_ms=med(t_kernel["hash"]), hash_ns_per_multiplication=round(hash_ns_per_mul, 6))
        for name, muls in (("fixed", MULS_FIXED), ("var", MULS_VAR)):
            kernel_ns = float(np.median(t_kernel[name])) * 1e6 / count
            line.update({name + "_call_ms": med(t_call[name]), name + "_kernel_ms": med(t_kernel[name]),
                         name + "_points_per_s": round(count / float(np.median(t_call[name])) * 1e3, 1),
                         name + "_ns_per_point_kernel": round(kernel_ns, 3), name + "_multiplications_per_point": muls,
                         name + "_of_yardstick": round(kernel_ns / (muls * hash_ns_per_mul), 3)})
        emit(line)
        del d_s, d_small, d_p, d_fixed, d_var, d_hash, d_gen
        torch.cuda.empty_cache()

    # ---- secrets -> keys -> leaves -> tree ----
    depth = args.chain_log
    count = 1 << depth
    d_s = drawn_words(torch, count, 99)
    d_keys = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
    d_leaves = torch.zeros((count, 4), dtype=torch.int64, device="cuda")
    trees = []

    def chain():
        ctx.babyjub_mul_batch(d_s.data_ptr(), None, count, d_keys.data_ptr(), 0)
        ctx.poseidon_hash_batch(d_keys.data_ptr(), 2, count, d_leaves.data_ptr())
        trees.append(ctx.poseidon_tree(d_leaves.data_ptr(), depth, n_leaves=count))

    clocked(chain)
    root = trees[0].root
    t_chain = []
    for _ in range(args.reps):
        trees.pop().close()
        t_chain.append(clocked(chain))
    k0 = int(zk.limbs_to_ints(d_s[:1].cpu().numpy().view(np.uint64))[0])
    key0 = tuple(zk.limbs_to_ints(d_keys[:1].cpu().numpy().view(np.uint64).reshape(2, 4)))
    emit(dict(tool="time_babyjub", what="chain", n=count, depth=depth, reps=args.reps, match=bool(trees[0].root == root and key0 == babyjub.mul(k0)),
              chain_ms=med(t_chain), identities_per_s=round(count / float(np.median(t_chain)) * 1e3, 1)))
    if out:
        out.close()


if __name__ == "__main__":
    main()
