"""Times the mixed witness path (zk_mixgen_run, csrc/mixgen.hip) against the tape it replaces and the boolean floor under it, in one
process, legs alternated: one JSON line per measurement.

    python tools/time_mixgen.py [--rounds 24,2] [--tails 1,16,1024] [--counts 64,4096,24768] [--reps 5] [--out profiles/mixgen.jsonl]

Circuit: SHA3-256 of a 64-byte message at `rounds` rounds, the digest packed into 2 wires of 128 bits (lo, hi), one field input c and
a tail of k general sub-circuits t0 = (lo + c) hi, t' = t (t + lo); the last tail wire and the two packs are public.  A batch cycles
through 64 messages and 64 values of c.  At 2 rounds the largest count is 65536 instead of 24768.

    mixgen    zk_mixgen_run on that circuit, host clock around the call (complete on return), and the k_mix_tail launches alone
              (device events, option "profile" = 2, in runs of their own)
    witgen    zk_witgen_run on the same circuit: the yardstick
    boolgen   zk_boolgen_run on the same circuit without the tail and the field input: the floor

After one warm-up of each leg the legs alternate `reps` times; medians with min and max.  `match`: every leg's first 64 witnesses equal
zk_circuit_weights word for word, and the packed digests equal hashlib.sha3_256 (24 rounds) or the floor's (fewer)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zksnark_rs_amd as zk  # noqa: E402
from zksnark_rs_amd.circuit import Boolgen, Builder, Mixgen, Witgen  # noqa: E402

DISTINCT = 64
MSG_BYTES = 64


def med(xs):
    return dict(median=round(float(np.median(xs)), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def circuit(rounds, k):
    """k == 0: the floor (no field input, no tail)"""
    b = Builder()
    msg = b.new_bits(8 * MSG_BYTES)
    c_in = b.new_wire() if k else None
    lo, hi = b.pack_bytes(b.keccak(msg, 136, 0x06, rounds, 32))
    if not k:
        return b.finish([lo, hi])
    t = b.new_sub_circuit([(1, lo), (1, c_in)], [(1, hi)])
    for _ in range(k - 1):
        t = b.new_sub_circuit([(1, t)], [(1, t), (1, lo)])
    return b.finish([t, lo, hi])


def clocked(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", default="24,2")
    ap.add_argument("--tails", default="1,16,1024")
    ap.add_argument("--counts", default="64,4096,24768")
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

    rng = np.random.default_rng(2026)
    msgs = rng.integers(0, 256, size=(DISTINCT, MSG_BYTES), dtype=np.uint8)
    srng = zk.SplitMix64(9)
    c_vals = zk.ints_to_limbs([0, 1, zk.R_MODULUS - 1] + [srng.fr() for _ in range(DISTINCT - 3)]).reshape(DISTINCT, 1, 4)
    bit_limbs = np.zeros((DISTINCT, 8 * MSG_BYTES, 4), np.uint64)
    bit_limbs[:, :, 0] = np.unpackbits(msgs, axis=1, bitorder="little")
    tape_inputs = np.concatenate([bit_limbs, c_vals], axis=1)          # creation order: the message bits, then c
    d_msgs = torch.from_numpy(msgs).cuda()
    d_c = torch.from_numpy(c_vals.view(np.int64)).cuda()
    d_tape = torch.from_numpy(tape_inputs.view(np.int64)).cuda()
    sha3 = [[int.from_bytes(hashlib.sha3_256(bytes(m)).digest()[16 * i:16 * i + 16], "little") for i in range(2)] for m in msgs]

    for rounds in [int(s) for s in args.rounds.split(",") if s]:
        floor = circuit(rounds, 0)
        bg = Boolgen(ctx, floor)
        want_floor = np.stack([floor.weights(bit_limbs[j]) for j in range(DISTINCT)])
        digests = zk.limbs_to_ints(want_floor[:, 1:3, :].reshape(-1, 4))
        digest_ok = rounds != 24 or digests == [v for row in sha3 for v in row]
        for k in [int(s) for s in args.tails.split(",") if s]:
            c = circuit(rounds, k)
            dims = c.mixed_dims()
            mg, wg = Mixgen(ctx, c), Witgen(ctx, c)
            want = np.stack([c.weights(tape_inputs[j]) for j in range(DISTINCT)])
            digest_k = digest_ok and zk.limbs_to_ints(want[:, 2:4, :].reshape(-1, 4)) == digests
            for count in [int(s) for s in args.counts.split(",") if s]:
                if rounds != 24 and count == 24768:
                    count = 65536
                base = dict(tool="time_mixgen", circuit="sha3_256_64B+tail", rounds=rounds, tail_sub_circuits=k, count=count, distinct_inputs=DISTINCT,
                            reps=args.reps, m=c.m, n=c.n, m_floor=floor.m, tail_share_of_gates=round(k / c.n, 6), **dims)
                if count * c.m * 32 > 0.7 * torch.cuda.mem_get_info()[0]:
                    emit(dict(base, skipped="device memory: %.1f GB of witnesses" % (count * c.m * 32 / 1e9)))
                    continue
                idx = torch.arange(count, device="cuda") % DISTINCT
                d_in, d_f, d_t = d_msgs[idx].contiguous(), d_c[idx].contiguous(), d_tape[idx].contiguous()
                d_out = torch.empty((count, c.m, 4), dtype=torch.int64, device="cuda")       # one buffer, the three legs in turn
                legs = {"mixgen": (lambda: mg.run(d_in.data_ptr(), d_f.data_ptr(), count, d_out.data_ptr()), c.m, want),
                        "witgen": (lambda: wg.run(d_t.data_ptr(), count, d_out.data_ptr()), c.m, want),
                        "boolgen": (lambda: bg.run(d_in.data_ptr(), count, d_out.data_ptr()), floor.m, want_floor)}

                def tail_kernel():
                    ctx.set_option("profile", 2)
                    ctx.profile_reset()
                    legs["mixgen"][0]()
                    prof = ctx.profile()
                    ctx.set_option("profile", 0)
                    return prof["mixgen_tail"]["total_ms"]

                match = bool(digest_k)
                for name, (call, m, ref) in legs.items():                                     # warm-up and check
                    d_out.zero_()
                    clocked(call)
                    n = min(DISTINCT, count)
                    got = d_out.view(-1)[:count * m * 4].view(count, m, 4)[:n].cpu().numpy().view(np.uint64)
                    match = match and bool(np.array_equal(got, ref[:n]))
                tail_kernel()
                t = {name: [] for name in legs}
                t["tail_kernel"] = []
                for _ in range(args.reps):
                    for name, (call, _, _) in legs.items():
                        t[name].append(clocked(call))
                    t["tail_kernel"].append(tail_kernel())
                mix, tape, flo = (float(np.median(t[x])) for x in ("mixgen", "witgen", "boolgen"))
                emit(dict(base, match=match, mixgen_ms=med(t["mixgen"]), witgen_ms=med(t["witgen"]), boolgen_floor_ms=med(t["boolgen"]),
                          tail_kernel_ms=med(t["tail_kernel"]), witgen_over_mixgen=round(tape / mix, 3), mixgen_over_floor=round(mix / flo, 4),
                          mixgen_witnesses_per_s=round(count / mix * 1e3, 1), witgen_witnesses_per_s=round(count / tape * 1e3, 1),
                          floor_witnesses_per_s=round(count / flo * 1e3, 1)))
                del d_in, d_f, d_t, d_out
                torch.cuda.empty_cache()
            mg.close()
            wg.close()
            c.close()
        bg.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
