"""Times the three ways from inputs to witnesses in HBM, and witness generation feeding the batched prover, in one process: one JSON
line per (gates, count).

    python tools/time_witgen.py [--gates 16,1024,65536] [--counts 64,4096,65536] [--reps 5] [--scratch-kib K] [--out profiles/witgen.jsonl]

Circuit: the chain written as .zk text (circuits.chain_zk; m = 2 n + 2).  A batch of `count` cycles through 64 distinct input sets.

    host       `count` calls of zk_circuit_weights into one host array, then the upload (the only path before the tape)
    host_tape  the same through zk_circuit_weights_tape
    gpu        zk_witgen_run, inputs resident in HBM
    gpu_prove  zk_witgen_run, then zk_prove_batch_submit over its output in batches of 64, two tickets in flight

Every clock stops after a device synchronise (the witgen and prove calls are complete on return; the uploads are followed by
torch.cuda.synchronize).  After one warm-up of each variant the variants alternate `reps` times; medians with min and max.  A pair is
skipped (`skipped`) when inputs plus witnesses do not fit in device memory or 64 instances do not fit the scratch cap; a variant whose
`count` calls would take more than ten seconds is not run in full: the host variants then time a sample of calls (`host_calls_timed`
< count, totals null, per-call figures measured), gpu_prove is left out (null).  `match`: the device witnesses of the first 64
instances equal zk_circuit_weights word for word."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd.circuit import Circuit, Witgen  # noqa: E402
from zksnark_rs_amd.circuits import chain_rows, chain_zk  # noqa: E402

DISTINCT = 64
LIMIT_S = 10.0
BATCH = zk._lib.MAX_BATCH


def med(xs):
    return dict(median=round(float(np.median(xs)), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def host_variant(fn, ins, count, calls, torch):
    """`calls` calls of fn over the cycled inputs into one array, then its upload; (ms of the calls, ms of the upload)"""
    t0 = time.perf_counter()
    out = np.stack([fn(ins[j % DISTINCT]) for j in range(calls)])
    t1 = time.perf_counter()
    d = torch.from_numpy(out.view(np.int64)).cuda()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    del d
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--gates", default="16,1024,65536")
    ap.add_argument("--counts", default="64,4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scratch-kib", type=int, default=None, help="option witgen_scratch_kib for this run (default: the library's 8 GiB)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = zk.Context(0)
    if args.scratch_kib is not None:
        ctx.set_option("witgen_scratch_kib", args.scratch_kib)
    out = open(args.out, "w") if args.out else None
    free_bytes = torch.cuda.mem_get_info()[0]
    cap_bytes = ctx.get_option("witgen_scratch_kib") * 1024

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    for n in [int(s) for s in args.gates.split(",") if s]:
        log_n = n.bit_length() - 1
        assert n == 1 << log_n
        c = Circuit(chain_zk(n))
        dims = c.tape_dims()
        rng = np.random.default_rng(n)
        ins = rng.integers(0, 1 << 63, size=(DISTINCT, c.n_in, 4), dtype=np.uint64)
        ins[:, :, 3] &= np.uint64((1 << 60) - 1)            # < 2^252 < r
        d_distinct = torch.from_numpy(ins.view(np.int64)).cuda()
        wg = Witgen(ctx, c)
        m_, l_, u, v, w = chain_rows(log_n)
        assert m_ == c.m
        qap = ctx.qap_sparse(log_n, m_, l_, u, v, w)
        srng = zk.SplitMix64(n)
        crs = ctx.setup(qap, [srng.fr() for _ in range(5)])
        rs, ss = [srng.fr() for _ in range(BATCH)], [srng.fr() for _ in range(BATCH)]
        want = np.stack([c.weights(ins[j]) for j in range(DISTINCT)])
        for count in [int(s) for s in args.counts.split(",") if s]:
            base = dict(tool="time_witgen", circuit="chain_zk", gates=n, m=c.m, n_in=c.n_in, count=count, distinct_inputs=DISTINCT,
                        reps=args.reps, scratch_kib=cap_bytes // 1024, tape_ops=dims["ops"], tape_slots=dims["slots"], depth=dims["depth"], width=dims["width"])
            group_bytes = dims["slots"] * 64 * 32
            need = count * (c.n_in + c.m) * 32 + min(cap_bytes, group_bytes * ((count + 63) // 64))
            if group_bytes > cap_bytes or need > 0.8 * free_bytes:
                emit(dict(base, skipped="device memory: %.1f GB needed" % (need / 1e9)))
                continue
            d_in = d_distinct[torch.arange(count, device="cuda") % DISTINCT].contiguous()
            d_out = torch.empty((count, c.m, 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()

            def gpu():
                t0 = time.perf_counter()
                wg.run(d_in.data_ptr(), count, d_out.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            def gpu_prove(limit=None):
                """-> ms; with `limit`, only that many batches (to estimate the whole)"""
                t0 = time.perf_counter()
                wg.run(d_in.data_ptr(), count, d_out.data_ptr())
                pending = []
                starts = list(range(0, count, BATCH))[:limit]
                for j0 in starts:
                    k = min(BATCH, count - j0)
                    ptrs = [d_out.data_ptr() + (j0 + j) * c.m * 32 for j in range(k)]
                    pending.append((ctx.prove_batch_submit(crs, qap, ptrs, [c.m] * k, rs[:k], ss[:k]), k))
                    if len(pending) == 2:
                        ctx.prove_batch_wait(*pending.pop(0))
                for p in pending:
                    ctx.prove_batch_wait(*p)
                return (time.perf_counter() - t0) * 1e3

            # warm-up of every variant; the first calls also size the full runs
            gpu()
            t_gen = gpu()
            k = min(DISTINCT, count)
            match = bool(np.array_equal(d_out[:k].cpu().numpy().view(np.uint64), want[:k]))
            per_call = host_variant(c.weights, ins, count, 2, torch)[0] / 2
            host_variant(c.weights_tape, ins, count, 2, torch)
            calls = count if per_call * count <= LIMIT_S * 1e3 else max(8, int(2e3 / per_call))
            calls = min(calls, count)
            nb = (count + BATCH - 1) // BATCH
            t_some = gpu_prove(limit=min(nb, 2))
            prove_full = t_gen + max(t_some - t_gen, 0.0) / min(nb, 2) * nb <= LIMIT_S * 1e3
            t = dict(host=[], host_up=[], tape=[], tape_up=[], gpu=[], gpu_prove=[])
            for _ in range(args.reps):
                a, b = host_variant(c.weights, ins, count, calls, torch)
                t["host"].append(a); t["host_up"].append(b)
                a, b = host_variant(c.weights_tape, ins, count, calls, torch)
                t["tape"].append(a); t["tape_up"].append(b)
                t["gpu"].append(gpu())
                if prove_full:
                    t["gpu_prove"].append(gpu_prove())
            full = calls == count
            g = float(np.median(t["gpu"]))
            hp, tp = float(np.median(t["host"])) / calls, float(np.median(t["tape"])) / calls
            line = dict(base, match=match, host_calls_timed=calls,
                        host_ms_per_call=round(hp, 5), host_tape_ms_per_call=round(tp, 5), tape_over_host=round(hp / tp, 2),
                        host_total_ms=med([x + y for x, y in zip(t["host"], t["host_up"])]) if full else None,
                        host_tape_total_ms=med([x + y for x, y in zip(t["tape"], t["tape_up"])]) if full else None,
                        gpu_ms=med(t["gpu"]), gpu_witnesses_per_s=round(count / g * 1e3, 1), gpu_ms_per_witness=round(g / count, 5),
                        gpu_over_host_tape_per_witness=round(tp / (g / count), 2),
                        gpu_prove_ms=med(t["gpu_prove"]) if prove_full else None,
                        gpu_prove_proofs_per_s=round(count / float(np.median(t["gpu_prove"])) * 1e3, 1) if prove_full else None)
            emit(line)
            del d_in, d_out
            torch.cuda.empty_cache()
        wg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
