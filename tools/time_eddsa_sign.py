"""Times EdDSA-Poseidon batch signing on the device (csrc/eddsa.hip, zk_eddsa_sign_batch) in one process, legs alternated: one JSON line
per size.

    python tools/time_eddsa_sign.py [--logs 10,16,20] [--host-sample 256] [--reps 5] [--out profiles/eddsa_sign.jsonl]

    sign          zk_eddsa_sign_batch on 2^k instances over drawn keys, nonce keys and messages, all distinct, resident on the device:
                  the host clock around the call (complete on return) and its kernels by device events (option "profile" = 2) in
                  runs of their own, together and each of the three alone
    fixed_k,      the work it is made of, in the same run: zk_babyjub_mul_batch fixed base on the same k, then on the same rho (rho is
    fixed_rho,    recovered on the host as S - 8 (hm mod l) k mod l from what signing wrote, and [rho] Base8 must be the R8 signing wrote),
    verify        and zk_eddsa_verify_batch on the produced signatures, whose first launch is the H6 kernel
    host          single-thread zk_eddsa_sign over the first `--host-sample` instances; they must equal the device's

The legs alternate `reps` times after one warm-up each.  `sign_over_parts`: the median of the sign call's kernels over the sum of the
two mul_batch kernel medians and twice the H6 kernel median.  `match`: every produced signature verifies VALID on the device, the
fixed-base results are the A and R8 of the rows, and the host sample agrees word for word."""
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

L = babyjub.params()["order"]
SIGN_KERNELS = ("eddsa_sign_nonce", "eddsa_sign_points", "eddsa_sign_response")


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


def drawn(count, seed=13):
    """(count, 4) uint64 each: keys in [1, 2^250), nonce keys and messages below 2^253 -- in range, and distinct but for a collision of 250 bits"""
    rng = np.random.default_rng(seed)
    k, n, m = [rng.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64) for _ in range(3)]
    k[:, 3] >>= np.uint64(6)
    k[:, 0] |= np.uint64(1)
    n[:, 3] >>= np.uint64(3)
    m[:, 3] >>= np.uint64(3)
    return k, n, m


def to_ints(words):
    raw = np.ascontiguousarray(words, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[32 * j:32 * j + 32], "little") for j in range(len(raw) // 32)]


def to_words(ints):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in ints), np.uint64).reshape(-1, 4).copy()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="10,16,20")
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

    for log_count in [int(x) for x in args.logs.split(",") if x]:
        count = 1 << log_count
        k, n, m = drawn(count)
        dev = lambda a: torch.from_numpy(a.view(np.int64)).to("cuda")                       # noqa: E731
        d_k, d_n, d_m = dev(k), dev(n), dev(m)
        d_p = torch.zeros((count, 20), dtype=torch.int64, device="cuda")
        d_s = torch.zeros((count, 4), dtype=torch.int64, device="cuda")
        d_bits = torch.zeros((count, 64), dtype=torch.uint8, device="cuda")
        d_st = torch.full((count,), -1, dtype=torch.int32, device="cuda")
        d_a = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
        d_r = torch.zeros((count, 8), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        sign = lambda: ctx.eddsa_sign_batch(d_k.data_ptr(), d_n.data_ptr(), d_m.data_ptr(), count, d_p.data_ptr(), d_s.data_ptr())   # noqa: E731
        ctx.eddsa_sign_batch(d_k.data_ptr(), d_n.data_ptr(), d_m.data_ptr(), count, d_p.data_ptr(), d_s.data_ptr(), d_bits.data_ptr(), 64)
        # rho = S - 8 (hm mod l) k mod l on the host, from S and the hm bits signing wrote
        rows = np.frombuffer(d_bits.cpu().numpy().tobytes(), np.uint8).reshape(count, 64)
        whole = [int.from_bytes(rows[j].tobytes(), "little") for j in range(count)]
        s_ints, k_ints = to_ints(d_s.cpu().numpy().view(np.uint64)), to_ints(k)
        rho = [(s - 8 * ((w >> eddsa.S_BITS) % L) * kk) % L for s, w, kk in zip(s_ints, whole, k_ints)]
        bits_agree = all(w & ((1 << eddsa.S_BITS) - 1) == s for s, w in zip(s_ints, whole))
        d_rho = dev(to_words(rho))
        torch.cuda.synchronize()
        legs = {"sign": (sign, "eddsa_sign"),
                "fixed_k": (lambda: ctx.babyjub_mul_batch(d_k.data_ptr(), None, count, d_a.data_ptr(), 0), "babyjub_mul_fixed"),
                "fixed_rho": (lambda: ctx.babyjub_mul_batch(d_rho.data_ptr(), None, count, d_r.data_ptr(), 0), "babyjub_mul_fixed"),
                "verify": (lambda: ctx.eddsa_verify_batch(d_p.data_ptr(), d_s.data_ptr(), count, d_st.data_ptr()), "eddsa_challenge")}
        for call, prefix in legs.values():
            clocked(call)
            profiled(ctx, call, prefix)
        t_call, t_kernel = {name: [] for name in legs}, {name: [] for name in legs}
        t_part = {name: [] for name in SIGN_KERNELS}                 # the sign call's launches, each alone
        for _ in range(args.reps):
            for name, (call, prefix) in legs.items():
                t_call[name].append(clocked(call))
                t_kernel[name].append(profiled(ctx, call, prefix))
            for name in t_part:
                t_part[name].append(profiled(ctx, sign, name))
        all_valid = bool((d_st == eddsa.VALID).all().item())
        points = d_p.view(count, 5, 4)
        parts_agree = bool(torch.equal(d_a.view(count, 2, 4), points[:, 0:2]) and torch.equal(d_r.view(count, 2, 4), points[:, 2:4]))
        sample = min(count, args.host_sample)
        n_ints, m_ints = to_ints(n[:sample]), to_ints(m[:sample])
        t0 = time.perf_counter()
        host = [eddsa.sign(kk, nn, mm) for kk, nn, mm in zip(k_ints[:sample], n_ints, m_ints)]
        host_us = (time.perf_counter() - t0) * 1e6 / sample          # through ctypes: the binding's per-call cost is inside
        got_rows = d_p[:sample].cpu().numpy().view(np.uint64).reshape(sample, 5, 4)
        host_agrees = all(tuple(zk.limbs_to_ints(got_rows[j, 2:4])) == host[j][0] and s_ints[j] == host[j][1] for j in range(sample))
        parts = float(np.median(t_kernel["fixed_k"])) + float(np.median(t_kernel["fixed_rho"])) + 2 * float(np.median(t_kernel["verify"]))
        line = dict(tool="time_eddsa_sign", what="sign_batch", count=count, reps=args.reps,
                    match=bool(all_valid and parts_agree and bits_agree and host_agrees),
                    host_single_thread_us_per_sign=round(host_us, 1), host_sample=sample)
        for name in legs:
            line.update({name + "_call_ms": med(t_call[name]), name + ("_h6_kernel_ms" if name == "verify" else "_kernel_ms"): med(t_kernel[name])})
        for name in SIGN_KERNELS:
            line[name[len("eddsa_sign_"):] + "_kernel_ms"] = med(t_part[name])
        line.update(signatures_per_s=round(count / float(np.median(t_call["sign"])) * 1e3, 1), parts_kernels_ms=round(parts, 4),
                    sign_over_parts=round(float(np.median(t_kernel["sign"])) / parts, 3))
        emit(line)
        del d_k, d_n, d_m, d_p, d_s, d_bits, d_st, d_a, d_r, d_rho
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
