"""Times EdDSA-Poseidon verification on the device (csrc/eddsa.hip) in one process, legs alternated: one JSON line per measurement.

    python tools/time_eddsa.py [--logs 10,16,20] [--signed 4096] [--host-sample 256] [--reps 5] [--chain-count 16] [--out profiles/eddsa.jsonl]

    verify_batch   zk_eddsa_verify_batch on 2^k signatures resident on the device -- `--signed` signatures made on the host over drawn
                   keys and messages, tiled -- next to the way to the same two scalar multiplications without it: zk_babyjub_mul_batch
                   fixed base on the S, then variable base on (hm, A), hm computed beforehand.  The three legs alternate `reps` times
                   after one warm-up each: host clock around the call (complete on return) and the kernels alone (device events, option
                   "profile" = 2, in runs of their own; the verify call's two launches also each alone).  `fused_over_two_calls`: the
                   verify call's median over the sum of the two mul_batch medians.  Single-thread zk_eddsa_verify on the host over the first `--host-sample` signatures.
    chain          zk_eddsa_verify_batch with bit rows -> zk_mixgen_run -> zk_prove_batch_submit / _wait on `--chain-count` signatures,
                   device to device, end to end by the host clock, in proofs/s; setup is outside the clock

`match`: every status is VALID, one planted wrong message gives MISMATCH, and the chain's proofs verify."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd import babyjub, eddsa  # noqa: E402
from zksnark_rs_amd.circuit import Builder, Mixgen  # noqa: E402

L = babyjub.params()["order"]


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


def signed(n, seed=7):
    """n signatures over drawn keys and messages -> (points (n, 5, 4), S (n, 4), hm (n, 4)) uint64, and the tuples"""
    rng = zk.SplitMix64(seed)
    sigs = []
    for _ in range(n):
        k, msg = rng.fr() % L or 1, rng.fr()
        r8, s = eddsa.sign(k, rng.fr(), msg)
        sigs.append((eddsa.public_key(k), msg, r8, s))
    points = np.stack([zk.ints_to_limbs([a[0], a[1], r8[0], r8[1], msg]) for a, msg, r8, _ in sigs])
    s = babyjub.scalars_to_words([s for _, _, _, s in sigs])
    hm = babyjub.scalars_to_words([eddsa.challenge(r8, a, msg) for a, msg, r8, _ in sigs])
    return points, s, hm, sigs


def tiled(torch, a, count):
    reps = -(-count // a.shape[0])
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([a] * reps)[:count]).view(np.int64)).to("cuda")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="10,16,20")
    ap.add_argument("--signed", type=int, default=4096)
    ap.add_argument("--host-sample", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chain-count", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = zk.Context(0)
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    points, s, hm, sigs = signed(args.signed)
    for log_count in [int(x) for x in args.logs.split(",") if x]:
        count = 1 << log_count
        d_p, d_s, d_hm = tiled(torch, points, count), tiled(torch, s, count), tiled(torch, hm, count)
        d_a = d_p[:, 0:2].contiguous().view(count, 8)
        d_st = torch.zeros(count, dtype=torch.int32, device="cuda")
        d_fixed = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
        d_var = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        legs = {"verify": (lambda: ctx.eddsa_verify_batch(d_p.data_ptr(), d_s.data_ptr(), count, d_st.data_ptr()), "eddsa"),
                "fixed": (lambda: ctx.babyjub_mul_batch(d_s.data_ptr(), None, count, d_fixed.data_ptr(), 0), "babyjub_mul_fixed"),
                "var": (lambda: ctx.babyjub_mul_batch(d_hm.data_ptr(), d_a.data_ptr(), count, d_var.data_ptr(), 0), "babyjub_mul_var")}
        for call, prefix in legs.values():
            clocked(call)
            profiled(ctx, call, prefix)
        t_call, t_kernel = {k: [] for k in legs}, {k: [] for k in legs}
        t_part = {"eddsa_challenge": [], "eddsa_curve": []}          # the verify call's two launches, each alone
        for _ in range(args.reps):
            for name, (call, prefix) in legs.items():
                t_call[name].append(clocked(call))
                t_kernel[name].append(profiled(ctx, call, prefix))
            for prefix in t_part:
                t_part[prefix].append(profiled(ctx, legs["verify"][0], prefix))
        all_valid = bool((d_st == 0).all().item())
        d_p[count // 2, 4, 0] ^= 1                              # another message under one signature
        torch.cuda.synchronize()
        ctx.eddsa_verify_batch(d_p.data_ptr(), d_s.data_ptr(), count, d_st.data_ptr())
        planted = d_st.cpu().numpy()
        one_mismatch = bool(planted[count // 2] == eddsa.MISMATCH and int((planted != 0).sum()) == 1)
        sample = min(count, args.host_sample, len(sigs))
        t0 = time.perf_counter()
        host = [eddsa.verify(a, msg, r8, sv) for a, msg, r8, sv in sigs[:sample]]
        host_us = (time.perf_counter() - t0) * 1e6 / sample         # through ctypes: the binding's per-call cost is inside
        two = float(np.median(t_call["fixed"])) + float(np.median(t_call["var"]))
        two_kernel = float(np.median(t_kernel["fixed"])) + float(np.median(t_kernel["var"]))
        line = dict(tool="time_eddsa", what="verify_batch", count=count, reps=args.reps, distinct_signatures=len(sigs),
                    match=bool(all_valid and one_mismatch and all(x == eddsa.VALID for x in host)),
                    host_single_thread_us_per_verify=round(host_us, 1), host_sample=sample)
        for name in legs:
            line.update({name + "_call_ms": med(t_call[name]), name + "_kernel_ms": med(t_kernel[name])})
        line.update(challenge_kernel_ms=med(t_part["eddsa_challenge"]), curve_kernel_ms=med(t_part["eddsa_curve"]))
        line.update(signatures_per_s=round(count / float(np.median(t_call["verify"])) * 1e3, 1),
                    two_calls_ms=round(two, 4), fused_over_two_calls=round(float(np.median(t_call["verify"])) / two, 3),
                    fused_over_two_calls_kernels=round(float(np.median(t_kernel["verify"])) / two_kernel, 3))
        emit(line)
        del d_p, d_s, d_hm, d_a, d_st, d_fixed, d_var
        torch.cuda.empty_cache()

    # ---- verify -> mixgen -> prove ----
    n = args.chain_count
    if n:
        b = Builder()
        f = [b.new_wire() for _ in range(5)]
        s_bits, hm_bits = b.new_bits(eddsa.S_BITS), b.new_bits(eddsa.HM_BITS)
        b.eddsa_verify(f[0:2], f[2:4], f[4], s_bits, hm_bits)
        gates = b.dims()[1]
        c = b.finish([f[0], f[1], f[4]])
        qap = c.qap_sparse_unity(ctx)
        rng = zk.SplitMix64(11)
        crs = ctx.setup(qap, zk.ints_to_limbs([rng.fr() for _ in range(5)]))
        mg = Mixgen(ctx, c)
        d_p, d_s = tiled(torch, points, n), tiled(torch, s, n)
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_bits = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        d_w = torch.zeros((n, c.m, 4), dtype=torch.int64, device="cuda")
        rs, ss = [rng.fr() for _ in range(n)], [rng.fr() for _ in range(n)]
        proofs = []

        def chain():
            proofs.clear()
            ctx.eddsa_verify_batch(d_p.data_ptr(), d_s.data_ptr(), n, d_st.data_ptr(), d_bits.data_ptr(), 64)
            mg.run(d_bits.data_ptr(), d_p.data_ptr(), n, d_w.data_ptr(), in_stride=64)
            for first in range(0, n, 64):                       # a batch holds at most 64 proofs
                k = min(64, n - first)
                ticket = ctx.prove_batch_submit(crs, qap, [d_w.data_ptr() + j * c.m * 32 for j in range(first, first + k)], [c.m] * k,
                                                rs[first:first + k], ss[first:first + k])
                proofs.extend(ctx.prove_batch_wait(ticket, k))

        clocked(chain)
        t_chain = [clocked(chain) for _ in range(args.reps)]
        public = d_p[:, [0, 1, 4]].cpu().numpy().view(np.uint64)
        ok = bool((d_st == 0).all().item() and ctx.verify_batch(crs, public, proofs).all())
        emit(dict(tool="time_eddsa", what="chain", count=n, gates=gates, m=c.m, reps=args.reps, match=ok, chain_ms=med(t_chain),
                  proofs_per_s=round(n / float(np.median(t_chain)) * 1e3, 2)))
        mg.close()
        crs.close()
        qap.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
