"""Times what packed wires (zk_builder_pack) change on the bit-sliced witness path, in one process, legs alternated: one JSON line per
measurement.

    python tools/time_boolgen_pack.py [--counts 64,4096,24768] [--verify-n 4096] [--reps 5] [--out profiles/boolgen_pack.jsonl]

Circuit: SHA3-256 of a 64-byte message built with circuit.Builder, twice: `packed` names the digest as 2 packed verify wires of 128
bits (Builder.pack_bytes), `bits` as 256 verify bits (the circuit of tools/time_boolgen.py).  A batch cycles through 64 messages.

    (a) kind "run"      zk_boolgen_run on both circuits at 24 rounds, host clock around the call (complete on return), and the
                        k_bool_expand_packs launches alone (device events, option "profile" = 2, in runs of their own)
    (b) kind "verify"   zk_verify_batch and zk_vk_verify_batch over N proofs (32 distinct ones, cycled) of the same messages, the
                        2-input CRS of `packed` against the 256-input CRS of `bits`, at 2 rounds (n = 32768 in both)
    (c) kind "inputs"   the public inputs of a batch: zk_boolgen_eval_fields of the 2 packed wires against zk_boolgen_eval of the
                        256 digest bits, at 24 rounds

After one warm-up of each leg the legs alternate `reps` times; medians with min and max.  `match`: the first 64 witnesses equal
zk_circuit_weights word for word and the packed inputs equal hashlib.sha3_256; `accepted`: every proof verified."""
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
from zksnark_rs_amd.circuit import Boolgen, Builder  # noqa: E402

DISTINCT = 64
PROOFS = 32
MSG_BYTES = 64


def med(xs):
    return dict(median=round(float(np.median(xs)), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def sha3_circuit(rounds, packed):
    b = Builder()
    msg = b.new_bits(8 * MSG_BYTES)
    digest = b.keccak(msg, 136, 0x06, rounds, 32)
    return b.finish(b.pack_bytes(digest) if packed else [w for word in digest for w in word])


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
    ap.add_argument("--counts", default="64,4096,24768")
    ap.add_argument("--verify-n", type=int, default=4096)
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
    fr_inputs = np.zeros((DISTINCT, 8 * MSG_BYTES, 4), np.uint64)
    fr_inputs[:, :, 0] = np.unpackbits(msgs, axis=1, bitorder="little")
    d_msgs = torch.from_numpy(msgs).cuda()
    want_public = [[int.from_bytes(hashlib.sha3_256(bytes(m)).digest()[16 * k:16 * k + 16], "little") for k in range(2)] for m in msgs]

    # ---- (a) and (c): 24 rounds ----
    circuits = {name: sha3_circuit(24, name == "packed") for name in ("packed", "bits")}
    gens = {name: Boolgen(ctx, c) for name, c in circuits.items()}
    want = {name: np.stack([c.weights(fr_inputs[j]) for j in range(8)]) for name, c in circuits.items()}
    m_max = max(c.m for c in circuits.values())
    free_bytes = torch.cuda.mem_get_info()[0]
    for count in [int(s) for s in args.counts.split(",") if s]:
        base = dict(tool="time_boolgen_pack", circuit="sha3_256_64B", rounds=24, count=count, distinct_inputs=DISTINCT, reps=args.reps,
                    m_packed=circuits["packed"].m, m_bits=circuits["bits"].m, public_inputs_packed=circuits["packed"].input,
                    public_inputs_bits=circuits["bits"].input)
        if count * m_max * 32 > 0.7 * free_bytes:
            emit(dict(base, kind="run", skipped="device memory: %.1f GB of witnesses" % (count * m_max * 32 / 1e9)))
            continue
        idx = torch.arange(count, device="cuda") % DISTINCT
        d_in = d_msgs[idx].contiguous()
        d_out = torch.empty((count, m_max, 4), dtype=torch.int64, device="cuda")      # one buffer, both circuits in turn
        d_fields = torch.empty((count, 2, 4), dtype=torch.int64, device="cuda")
        d_bits = torch.empty((count, 32), dtype=torch.uint8, device="cuda")

        def run(name):
            return clocked(lambda: gens[name].run(d_in.data_ptr(), count, d_out.data_ptr()))

        def pack_kernel():
            ctx.set_option("profile", 2)
            ctx.profile_reset()
            gens["packed"].run(d_in.data_ptr(), count, d_out.data_ptr())
            prof = ctx.profile()
            ctx.set_option("profile", 0)
            return prof["boolgen_expand_packs"]["total_ms"], prof["boolgen_expand"]["total_ms"]

        match = True
        for name in ("bits", "packed"):                                               # warm-up and check
            run(name)
            k = min(8, count)
            c = circuits[name]
            got = d_out.view(-1)[:count * c.m * 4].view(count, c.m, 4)[:k].cpu().numpy().view(np.uint64)
            match = match and bool(np.array_equal(got, want[name][:k]))
        pack_kernel()
        t = dict(packed=[], bits=[], pack_kernel=[], expand_kernel=[])
        for _ in range(args.reps):
            t["packed"].append(run("packed"))
            t["bits"].append(run("bits"))
            pk, ex = pack_kernel()
            t["pack_kernel"].append(pk); t["expand_kernel"].append(ex)
        p_ms, b_ms = float(np.median(t["packed"])), float(np.median(t["bits"]))
        emit(dict(base, kind="run", match=match, packed_ms=med(t["packed"]), bits_ms=med(t["bits"]), packed_over_bits=round(p_ms / b_ms, 4),
                  packed_witnesses_per_s=round(count / p_ms * 1e3, 1), bits_witnesses_per_s=round(count / b_ms * 1e3, 1),
                  pack_kernel_ms=med(t["pack_kernel"]), expand_kernel_ms=med(t["expand_kernel"])))

        def fields():
            return clocked(lambda: gens["packed"].eval_fields(d_in.data_ptr(), count, [1, 2], d_fields.data_ptr()))

        def bits():
            return clocked(lambda: gens["bits"].eval(d_in.data_ptr(), count, range(1, 257), d_bits.data_ptr()))

        fields(); bits()
        k = min(DISTINCT, count)
        got = zk.limbs_to_ints(d_fields[:k].cpu().numpy().view(np.uint64).reshape(-1, 4))
        match = got == [v for row in want_public[:k] for v in row]
        match = match and all(bytes(d_bits[j].cpu().numpy()) == hashlib.sha3_256(bytes(msgs[j])).digest() for j in range(k))
        t = dict(fields=[], bits=[])
        for _ in range(args.reps):
            t["fields"].append(fields())
            t["bits"].append(bits())
        emit(dict(base, kind="inputs", match=bool(match), eval_fields_ms=med(t["fields"]), eval_bits_ms=med(t["bits"]),
                  fields_over_bits=round(float(np.median(t["fields"])) / float(np.median(t["bits"])), 4),
                  out_bytes_fields=count * 64, out_bytes_bits=count * 32))
        del d_in, d_out, d_fields, d_bits
        torch.cuda.empty_cache()
    for g in gens.values():
        g.close()

    # ---- (b): verification over the two CRSs, 2 rounds ----
    n_ver = args.verify_n
    legs = {}
    for name in ("packed", "bits"):
        c = sha3_circuit(2, name == "packed")
        bg = Boolgen(ctx, c)
        d_w = torch.empty((PROOFS, c.m, 4), dtype=torch.int64, device="cuda")
        bg.run(d_msgs.data_ptr(), PROOFS, d_w.data_ptr())
        public = bg.eval_fields_numpy(msgs[:PROOFS], range(1, c.input + 1))           # bits and packed wires alike: the `inputs` array
        qap = c.qap_sparse_unity(ctx)
        srng = zk.SplitMix64(2)
        crs = ctx.setup(qap, [srng.fr() for _ in range(5)])
        ptrs = [d_w.data_ptr() + j * c.m * 32 for j in range(PROOFS)]
        ticket = ctx.prove_batch_submit(crs, qap, ptrs, [c.m] * PROOFS, [srng.fr() for _ in range(PROOFS)], [srng.fr() for _ in range(PROOFS)])
        proofs = np.frombuffer(b"".join(ctx.prove_batch_wait(ticket, PROOFS)), np.uint8).reshape(PROOFS, -1)
        pick = np.arange(n_ver) % PROOFS
        legs[name] = dict(c=c, crs=crs, qap=qap, vk=ctx.verifying_key(crs), inputs=np.ascontiguousarray(public[pick]),
                          proofs=np.ascontiguousarray(proofs[pick]), n=qap.n)
        bg.close()
        del d_w
    calls = {"crs": lambda g: ctx.verify_batch(g["crs"], g["inputs"], g["proofs"]), "vk": lambda g: g["vk"].verify_batch(ctx, g["inputs"], g["proofs"])}
    accepted = all(bool(call(g).all()) for g in legs.values() for call in calls.values())                     # warm-up and check
    t = {(name, key): [] for name in legs for key in calls}
    for _ in range(args.reps):
        for key, call in calls.items():
            for name, g in legs.items():
                t0 = time.perf_counter()
                call(g)
                t[(name, key)].append((time.perf_counter() - t0) * 1e3)
    line = dict(tool="time_boolgen_pack", kind="verify", circuit="sha3_256_64B", rounds=2, n=legs["packed"]["n"], proofs=n_ver, distinct_proofs=PROOFS,
                reps=args.reps, accepted=accepted, public_inputs_packed=legs["packed"]["c"].input, public_inputs_bits=legs["bits"]["c"].input)
    for key in calls:
        for name in legs:
            line["%s_%s_ms" % (key, name)] = med(t[(name, key)])
        line["%s_packed_over_bits" % key] = round(float(np.median(t[("packed", key)])) / float(np.median(t[("bits", key)])), 4)
    emit(line)
    if out:
        out.close()


if __name__ == "__main__":
    main()
