"""Times bit-sliced witness generation (zk_boolgen_run) against the tape kernel (zk_witgen_run) on the SAME built circuit, the expansion
kernel against a memset of its output buffer, and generate-then-prove, in one process: one JSON line per (rounds, count).

    python tools/time_boolgen.py [--rounds 24,2] [--counts 64,4096,max] [--reps 5] [--group-words 0] [--expand-form F] [--out profiles/boolgen.jsonl]

Circuit: SHA3-256 of a 64-byte message built with circuit.Builder, the permutation cut to `rounds` rounds (24 = the real one).
A batch of `count` cycles through 64 distinct messages.  `max` = as many instances as fit in 60 % of the free device memory, at most
65536, rounded down to a multiple of 64.

    (a) boolgen     zk_boolgen_run, packed inputs resident in HBM        tape     zk_witgen_run, field-element inputs resident in HBM
        The tape kernel is the yardstick.  Where 64 instances of it do not fit its scratch cap, or one run takes (or, at the rate
        of the count before, would take) more than the time limit, `tape_ms` is null and `tape_skipped` says why.
    (b) expand      the k_bool_expand launches alone (device events, option "profile" = 2, in a run of their own) over the bytes
        they write, against hipMemsetAsync of the same buffer between two events on its stream, in the same process
    (c) gen_prove   zk_boolgen_run, then zk_prove_batch_submit over its output in batches of 64, two tickets in flight (2 rounds only)

Host clocks stop after a device synchronise (both run calls are complete on return).  After one warm-up of each leg the legs alternate
`reps` times; medians with min and max.  `match`: the first 64 witnesses equal zk_circuit_weights word for word and their digests
hashlib.sha3_256 (24 rounds)."""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd.circuit import Boolgen, Builder, Witgen  # noqa: E402

DISTINCT = 64
LIMIT_S = 20.0
BATCH = zk._lib.MAX_BATCH
MSG_BYTES = 64


def med(xs):
    return dict(median=round(float(np.median(xs)), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def sha3_circuit(rounds):
    b = Builder()
    msg = b.new_bits(8 * MSG_BYTES)
    digest = [w for word in b.keccak(msg, 136, 0x06, rounds, 32) for w in word]
    return b.finish(digest)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", default="24,2")
    ap.add_argument("--counts", default="64,4096,max")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--group-words", type=int, default=0, help="option boolgen_group_words for this run (0 = the library's rule)")
    ap.add_argument("--expand-form", type=int, default=None, help="option boolgen_expand_form for this run (default: the library's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = zk.Context(0)
    hip = ctypes.CDLL("libamdhip64.so")                     # already resident (torch's): only hipMemsetAsync is taken from it
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    out = open(args.out, "w") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()

    rng = np.random.default_rng(2026)
    msgs = rng.integers(0, 256, size=(DISTINCT, MSG_BYTES), dtype=np.uint8)
    bits = np.unpackbits(msgs, axis=1, bitorder="little")
    fr_inputs = np.zeros((DISTINCT, 8 * MSG_BYTES, 4), np.uint64)
    fr_inputs[:, :, 0] = bits
    d_msgs = torch.from_numpy(msgs).cuda()
    d_fr = torch.from_numpy(fr_inputs.view(np.int64)).cuda()
    for rounds in [int(s) for s in args.rounds.split(",") if s]:
        c = sha3_circuit(rounds)
        dims = c.tape_dims()
        bg = Boolgen(ctx, c, group_words=args.group_words or None, expand_form=args.expand_form)
        wg = Witgen(ctx, c)
        tape_cap = ctx.get_option("witgen_scratch_kib") * 1024
        tape_group = dims["slots"] * 64 * 32
        want = np.stack([c.weights(fr_inputs[j]) for j in range(DISTINCT)])
        qap = crs = None
        if rounds == 2:
            qap = c.qap_sparse_unity(ctx)
            srng = zk.SplitMix64(rounds)
            crs = ctx.setup(qap, [srng.fr() for _ in range(5)])
            rs, ss = [srng.fr() for _ in range(BATCH)], [srng.fr() for _ in range(BATCH)]
        free_bytes = torch.cuda.mem_get_info()[0]
        tape_ms_per_instance = None                          # from the count before: a tape run expected past the limit is not started
        for token in [s for s in args.counts.split(",") if s]:
            count = min(int(0.6 * free_bytes / (c.m * 32)), 65536) // 64 * 64 if token == "max" else int(token)
            base = dict(tool="time_boolgen", circuit="sha3_256_64B", rounds=rounds, gates=c.n, m=c.m, n_in=c.n_in, count=count,
                        distinct_inputs=DISTINCT, reps=args.reps, group_words=args.group_words,
                        expand_form=ctx.get_option("boolgen_expand_form") if args.expand_form is None else args.expand_form, tape_ops=dims["ops"], tape_slots=dims["slots"],
                        state_bytes_per_64=(c.m + 1) * 8, tape_scratch_bytes_per_64=tape_group, out_bytes=count * c.m * 32)
            if count < 1 or count * c.m * 32 > 0.7 * free_bytes:
                emit(dict(base, skipped="device memory"))
                continue
            idx = torch.arange(count, device="cuda") % DISTINCT
            d_in = d_msgs[idx].contiguous()
            d_out = torch.empty((count, c.m, 4), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()

            def boolgen():
                t0 = time.perf_counter()
                bg.run(d_in.data_ptr(), count, d_out.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            boolgen()
            k = min(DISTINCT, count)
            match = bool(np.array_equal(d_out[:k].cpu().numpy().view(np.uint64), want[:k]))
            if rounds == 24:
                dig = bg.eval_numpy(msgs[:k], range(1, 257))
                match = match and all(bytes(dig[j]) == hashlib.sha3_256(bytes(msgs[j])).digest() for j in range(k))

            # the tape leg: its own input array (32 bytes per input bit), the same output buffer
            tape_skipped, d_fr_in = None, None
            tape_need = count * c.n_in * 32 + min(tape_cap, tape_group * ((count + 63) // 64))
            if tape_group > tape_cap:
                tape_skipped = "64 instances need %.2f GiB of tape scratch, above witgen_scratch_kib" % (tape_group / 2 ** 30)
            elif tape_need + count * c.m * 32 > 0.85 * free_bytes:
                tape_skipped = "device memory: %.1f GB for the tape's inputs and scratch" % (tape_need / 1e9)
            elif tape_ms_per_instance is not None and tape_ms_per_instance * count > LIMIT_S * 1e3:
                tape_skipped = "expected %.0f s at the rate of the count before" % (tape_ms_per_instance * count / 1e3)
            else:
                d_fr_in = d_fr[idx].contiguous()
                torch.cuda.synchronize()

            def tape():
                t0 = time.perf_counter()
                wg.run(d_fr_in.data_ptr(), count, d_out.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            tape_once = None
            if tape_skipped is None:
                tape_once = tape()
                tape_match = bool(np.array_equal(d_out[:k].cpu().numpy().view(np.uint64), want[:k]))
                tape_ms_per_instance = tape_once / count
                if tape_once > LIMIT_S * 1e3:
                    tape_skipped = "one run took %.1f s (timed once)" % (tape_once / 1e3)

            def gen_prove():
                t0 = time.perf_counter()
                bg.run(d_in.data_ptr(), count, d_out.data_ptr())
                pending = []
                for j0 in range(0, count, BATCH):
                    kk = min(BATCH, count - j0)
                    ptrs = [d_out.data_ptr() + (j0 + j) * c.m * 32 for j in range(kk)]
                    pending.append((ctx.prove_batch_submit(crs, qap, ptrs, [c.m] * kk, rs[:kk], ss[:kk]), kk))
                    if len(pending) == 2:
                        ctx.prove_batch_wait(*pending.pop(0))
                for p in pending:
                    ctx.prove_batch_wait(*p)
                return (time.perf_counter() - t0) * 1e3

            prove = crs is not None and count <= 4096
            if prove:
                prove = gen_prove() <= LIMIT_S * 1e3

            def memset():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                assert hip.hipMemsetAsync(d_out.data_ptr(), 0, count * c.m * 32, None) == 0
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            def expand():
                ctx.set_option("profile", 2)
                ctx.profile_reset()
                bg.run(d_in.data_ptr(), count, d_out.data_ptr())
                prof = ctx.profile()
                ctx.set_option("profile", 0)
                return {name: prof[name]["total_ms"] for name in ("boolgen_load", "boolgen_eval", "boolgen_expand") if name in prof}

            memset()
            expand()
            t = dict(boolgen=[], tape=[], gen_prove=[], memset=[], load=[], eval=[], expand=[])
            for _ in range(args.reps):
                t["boolgen"].append(boolgen())
                if tape_skipped is None:
                    t["tape"].append(tape())
                if prove:
                    t["gen_prove"].append(gen_prove())
                t["memset"].append(memset())
                e = expand()
                t["load"].append(e.get("boolgen_load", 0.0)); t["eval"].append(e.get("boolgen_eval", 0.0)); t["expand"].append(e["boolgen_expand"])
            b_ms, x_ms, s_ms = float(np.median(t["boolgen"])), float(np.median(t["expand"])), float(np.median(t["memset"]))
            nbytes = count * c.m * 32
            line = dict(base, match=match, boolgen_ms=med(t["boolgen"]), boolgen_witnesses_per_s=round(count / b_ms * 1e3, 1),
                        tape_ms=med(t["tape"]) if t["tape"] else None, tape_skipped=tape_skipped,
                        tape_once_ms=round(tape_once, 3) if tape_once is not None else None,
                        tape_match=tape_match if tape_once is not None else None,
                        tape_over_boolgen=round(float(np.median(t["tape"])) / b_ms, 2) if t["tape"] else
                        (round(tape_once / b_ms, 2) if tape_once is not None else None),
                        load_kernel_ms=med(t["load"]), eval_kernel_ms=med(t["eval"]), expand_kernel_ms=med(t["expand"]),
                        expand_gb_per_s=round(nbytes / x_ms / 1e6, 1), memset_ms=med(t["memset"]), memset_gb_per_s=round(nbytes / s_ms / 1e6, 1),
                        expand_over_memset_rate=round(s_ms / x_ms, 3),
                        gen_prove_ms=med(t["gen_prove"]) if t["gen_prove"] else None,
                        gen_prove_proofs_per_s=round(count / float(np.median(t["gen_prove"])) * 1e3, 1) if t["gen_prove"] else None)
            emit(line)
            del d_in, d_out, d_fr_in
            torch.cuda.empty_cache()
        bg.close()
        wg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
