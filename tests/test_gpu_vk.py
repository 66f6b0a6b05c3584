"""-m gpu: a verifying key on the device (csrc/vk_batch.hip).  The input sums from the key's window tables (k_vk_table /
k_vk_inputs) against Python integers and against zk_verify_batch's bit-serial kernel on crafted keys; verdict parity of the
key's batch calls with the CRS calls and with the host zk_vk_verify; chunking, transport through bytes, the binding of a key to
one context, key / context tear-down in either order, a call next to an outstanding proof ticket, and the C++ layer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs, SplitMix64, _lib
from test_gpu_verify_batch import simple, _tampered_batch, wide_program, ROOT, ZK_DIR, CHUNK  # noqa: F401
from test_gpu_verify_batch_all import splitmix_z
from test_verify_all_device_code import g1_words, g2_words

R = zk.R_MODULUS
TABLE_BYTES_PER_INPUT = 64 * 15 * 64      # windows x entries x sizeof(G1A)


def crafted_key(a):
    """sum_gamma_i = a_i G (a_i = 0: infinity); alpha, beta, gamma, delta multiples of the generators"""
    import pyref
    mul = lambda k: None if k % R == 0 else pyref.g1_mul(pyref.G1_GEN, k % R)   # noqa: E731
    return zk.VerifyingKey.from_points(np.array(g1_words(mul(5)), np.uint64), np.array(g2_words(pyref.g2_mul(pyref.G2_GEN, 7)), np.uint64),
                                       np.array(g2_words(pyref.g2_mul(pyref.G2_GEN, 11)), np.uint64),
                                       np.array(g2_words(pyref.g2_mul(pyref.G2_GEN, 13)), np.uint64),
                                       np.array([g1_words(mul(ai)) for ai in a], np.uint64))


def expected_sums(a, rows):
    import pyref
    out = []
    for row in rows:
        k = (a[0] + sum(x * ai for x, ai in zip(row, a[1:]))) % R
        out.append(g1_words(None if k == 0 else pyref.g1_mul(pyref.G1_GEN, k)))
    return np.array(out, dtype=np.uint64)


def edge_values():
    """x = 0, 1, 15, 16, 2^(4s) and 2^(4s) - 1 at the window joins s = 1, 31, 63, r - 1, the largest value < r with every
    4-bit digit non-zero"""
    vals = [0, 1, 15, 16, R - 1]
    for s in (1, 31, 63):
        vals += [1 << (4 * s), (1 << (4 * s)) - 1]
    top = R >> 252                                  # the top window holds r's two top bits
    full = int("%x" % (top - 1) + "f" * 63, 16) if top > 1 else None
    assert full is not None and full < R and all((full >> (4 * s)) & 15 for s in range(64))
    vals.append(full)
    assert all(v < R for v in vals)
    return vals


def rows_for(l, n, seed):
    """n rows of l inputs.  Rows 0 .. 11 hold nothing but edge values, shifted by one per column, so that every edge value stands
    in every column once; behind them edge values (walking through all twelve in every column) alternate with seeded random ones"""
    rng = SplitMix64(seed)
    edges = edge_values()
    rows = [[edges[(e + i) % len(edges)] for i in range(l)] for e in range(min(n, len(edges)))]
    for j in range(len(rows), n):
        rows.append([edges[(j // 2 + 5 * i) % len(edges)] if (j + i) % 2 == 0 else rng.fr() for i in range(l)])
    return rows


def both_sums(ctx, key, rows):
    t1 = key.input_sums(ctx, rows, tables=True)
    t0 = key.input_sums(ctx, rows, tables=False)
    assert np.array_equal(t0, t1)
    return t1


@pytest.mark.gpu
@pytest.mark.parametrize("l", [1, 2, 3, 17])
def test_input_sums_against_python_integers(ctx, l):
    rng = SplitMix64(900 + l)
    a = [rng.fr() for _ in range(l + 1)]
    key = crafted_key(a)
    # one pool of 130 rows and its integers, computed once (a host scalar multiplication per row); every batch size is a prefix
    pool = rows_for(l, 130, 31 * l)
    edges = edge_values()
    for i in range(l):
        assert {r[i] for r in pool[:12]} == set(edges)          # every edge value in every column
    want = expected_sums(a, pool)
    for n in (63, 64, 65, 130):                     # the 64-lane block's edge, more than one block
        got_1 = key.input_sums(ctx, pool[:n], tables=True)
        got_0 = key.input_sums(ctx, pool[:n], tables=False)
        assert np.array_equal(got_1, want[:n]), (l, n)          # both kernels against the integers, every row
        assert np.array_equal(got_0, want[:n]), (l, n)
    for j in list(range(12)) + [12, 129]:           # N = 1: each all-edge row on its own, and two mixed ones
        got_1 = key.input_sums(ctx, pool[j:j + 1], tables=True)
        got_0 = key.input_sums(ctx, pool[j:j + 1], tables=False)
        assert np.array_equal(got_1, want[j:j + 1]) and np.array_equal(got_0, want[j:j + 1]), (l, j)
    # rows longer than l: the tail is never read; shorter: fewer bases
    rows = [r + [R + 9] for r in pool[10:15]]
    assert np.array_equal(both_sums(ctx, key, rows), want[10:15])
    if l > 1:
        short = [r[:l - 1] for r in pool[10:15]]
        assert np.array_equal(both_sums(ctx, key, short), expected_sums(a[:l], short))
    with pytest.raises(zk.ZkError) as e:
        key.input_sums(ctx, [[R] * l])
    assert e.value.status == _lib.ZK_ERR_RANGE
    assert key.input_sums(ctx, np.zeros((0, l, 4), np.uint64)).shape == (0, 8)


@pytest.mark.gpu
def test_input_sums_on_degenerate_keys(ctx):
    """equal bases, opposite bases (the running sum passes through infinity), a base at infinity, a_0 = 0, and rows whose sum is
    infinity: every special case of the complete mixed addition"""
    rng = SplitMix64(4711)
    b, c = rng.fr(), rng.fr()
    edges = edge_values()
    for a in ([c, b, b, 7],                         # two equal bases
              [c, b, R - b, b],                     # a_1 = -a_2
              [c, 0, b, 0],                         # bases at infinity
              [0, b, 1, 2],                         # a_0 = 0
              [0, 0, 0, 0]):                        # nothing but infinities
        key = crafted_key(a)
        rows = [[x, x, y] for x in edges[:6] for y in (0, 1, edges[-1])]
        rows += [[x, 1, 0] for x in edges] + [[1, x, 5] for x in edges]
        if a[1] % R:
            inv = pow(a[1], -1, R)
            rows.append([(-(a[0] + 3 * a[2] + 4 * a[3]) * inv) % R, 3, 4])     # S = infinity
            rows.append([(-a[0] * inv) % R, 0, 0])                            # S = infinity with the other digits all zero
        got = both_sums(ctx, key, rows)
        want = expected_sums(a, rows)
        assert np.array_equal(got, want), a
        if a[1] % R:
            assert not got[-1].any() and not got[-2].any()


def _build_case(ctx, qap, weights, l, seed, count=3):
    """(crs, the l public inputs as limbs, `count` honest proofs, one proof of the same witness under another CRS)"""
    rng = SplitMix64(seed)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    proofs = [ctx.prove(crs, qap, weights, rng.fr(), rng.fr()) for _ in range(count)]
    other = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    foreign = ctx.prove(other, qap, weights, rng.fr(), rng.fr())
    return dict(crs=crs, x=np.ascontiguousarray(weights[1:1 + l]), proofs=proofs, foreign=foreign)


def _program_case(ctx, code, inputs, seed, sparse=False):
    from zksnark_rs_amd.circuit import Circuit
    c = Circuit(code)
    return _build_case(ctx, c.qap_sparse(ctx) if sparse else c.qap(ctx), c.weights(inputs), c.input, seed)


@pytest.fixture(scope="module")
def wide(ctx):
    """the 257-input circuit of test_gpu_verify_batch.py: CRS, its key, three proofs, a foreign proof"""
    rng = SplitMix64(2570)
    case = _program_case(ctx, wide_program(256), [rng.fr() for _ in range(256)], 259, sparse=True)
    assert case["x"].shape[0] == 257
    return dict(case, key=ctx.verifying_key(case["crs"]))


@pytest.mark.gpu
def test_257_inputs_and_the_table_cap(ctx, wide):
    key, x, proofs = wide["key"], wide["x"], wide["proofs"]
    assert key.input == 257
    rng = SplitMix64(99)
    rows = np.stack([x, ints_to_limbs([rng.fr() for _ in range(257)]), ints_to_limbs(edge_values() * 26)[:257]])
    sums = both_sums(ctx, key, rows)
    prow = np.repeat(x[None], 3, axis=0)
    bad = rows.copy()
    want = np.array([True, False, False])
    assert np.array_equal(key.verify_batch(ctx, prow, proofs), [True] * 3)
    assert np.array_equal(key.verify_batch(ctx, bad, [proofs[0]] * 3), want)
    keep = ctx.get_option("vk_table_kib")
    assert keep == 65536
    table_kib = 257 * TABLE_BYTES_PER_INPUT // 1024
    try:
        for cap in (table_kib - 1, 0):
            ctx.set_option("vk_table_kib", cap)
            fresh = zk.VerifyingKey.from_bytes(key.to_bytes())     # never had tables
            for k in ((key,) if cap else (fresh,)):                  # a key that has tables under a smaller cap; one that never had any
                with pytest.raises(zk.ZkError) as e:
                    k.input_sums(ctx, rows, tables=True)
                assert e.value.status == _lib.ZK_ERR_SIZE
                assert np.array_equal(k.input_sums(ctx, rows, tables=False), sums)
                assert np.array_equal(k.verify_batch(ctx, bad, [proofs[0]] * 3), want)
                assert np.array_equal(k.verify_batch(ctx, prow, proofs), [True] * 3)
        ctx.set_option("vk_table_kib", table_kib)                  # exactly the table size: allowed
        assert np.array_equal(key.input_sums(ctx, rows, tables=True), sums)
    finally:
        ctx.set_option("vk_table_kib", keep)


def tampered_batch(case, seed):
    """test_gpu_verify_batch.py's _tampered_batch rebuilt over any case's own proofs and input row: (rows (N, l, 4), proofs),
    shuffled -- honest proofs, a changed first and a changed last input, A and C swapped, a proof under another CRS, B outside G2
    and B moved into G2, and per point: infinity with a zero tail, tag 0x00 with a tail, tag 0x04 with (0, 0), unknown tags, a
    coordinate == q; single flipped bits"""
    import pyref
    from test_verify import twist_point_outside_g2, g2_mul_raw
    x, proofs = case["x"], case["proofs"]
    p0, p1 = proofs[0], proofs[1]
    B_out = twist_point_outside_g2(seed)
    B_in = g2_mul_raw(B_out, 2 * pyref.Q - pyref.R)       # cofactor cleared: in G2, but not the proof's B
    q_words = pyref.Q.to_bytes(32, "big")
    first, last = x.copy(), x.copy()
    first[0, 0] ^= np.uint64(1)
    last[-1, 1] ^= np.uint64(4)
    cases = [(x, p) for p in proofs]
    cases += [(first, p0), (last, p1),                      # wrong public input
              (x, p0[194:] + p0[65:194] + p0[:65]),         # A and C swapped
              (x, case["foreign"]),                         # made under another CRS
              (x, p0[:65] + pyref.enc_g2(B_out) + p0[194:]),
              (x, p0[:65] + pyref.enc_g2(B_in) + p0[194:])]
    for off, size in ((0, 65), (65, 129), (194, 65)):
        cases.append((x, p0[:off] + bytes(size) + p0[off + size:]))                         # infinity, zero tail
        cases.append((x, p0[:off] + b"\x00" + p0[off + 1:]))                                 # tag 0x00, non-zero tail
        cases.append((x, p0[:off] + b"\x04" + bytes(size - 1) + p0[off + size:]))           # tag 0x04 with (0, 0)
        for tag in (1, 2, 3, 5, 0xff):
            cases.append((x, p0[:off] + bytes([tag]) + p0[off + 1:]))                        # unknown tags
        cases.append((x, p0[:off + 1] + q_words + p0[off + 33:]))                           # a coordinate == q
    for bit in (0, 9, 300, 1000, 1600, 2000):
        bad = bytearray(p1); bad[bit // 8] ^= 1 << (bit % 8)
        cases.append((x, bytes(bad)))                                                       # a single flipped bit
    order = np.random.default_rng(seed).permutation(len(cases))
    return np.stack([cases[i][0] for i in order]), [cases[i][1] for i in order]


def host_verdicts(key, rows, proofs):
    return np.array([key.verify(r, p) for r, p in zip(rows, proofs)], dtype=bool)


@pytest.fixture(scope="module")
def parity_cases(ctx, wide):
    """simple.zk (l = 2), deg_15.zk, the 2^10 chain and the 257-input circuit, each with its own proofs, built once"""
    from zksnark_rs_amd.circuit import Circuit
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    rng = SplitMix64(1516)
    cases = [_program_case(ctx, open(os.path.join(ZK_DIR, "simple.zk")).read(), [3, 2, 4], 2028)]
    code = open(os.path.join(ZK_DIR, "deg_15.zk")).read()
    cases.append(_program_case(ctx, code, [rng.fr() for _ in range(Circuit(code).n_in)], 18))
    log_n = 10
    m, l, u, v, w = chain_rows(log_n)
    weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    cases.append(_build_case(ctx, ctx.qap_sparse(log_n, m, l, u, v, w), weights, l, 1024))
    cases.append(wide)
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_verdict_parity_with_the_crs_calls(ctx, parity_cases, which):
    """vk.verify_batch == ctx.verify_batch == [vk.verify] on the honest proofs and on the whole tampered list of each circuit;
    the same for the compressed call (every entry that has a compressed form) and for verify_batch_all (honest batch -> 1, one
    bad proof -> 0, the two cancellation pairs with z = (1, 1) -> 1, with z = (1, 2) -> 0)"""
    import pyref
    from test_verify_all_device_code import _points
    case = parity_cases[which]
    crs, x, honest = case["crs"], case["x"], case["proofs"]
    key = ctx.verifying_key(crs)
    rng = SplitMix64(5 + which)
    h_rows = np.repeat(x[None], len(honest), axis=0)
    t_rows, t_proofs = tampered_batch(case, 5 + which)
    for rows, proofs, all_good in ((h_rows, honest, True), (t_rows, t_proofs, False)):
        got = key.verify_batch(ctx, rows, proofs)
        assert np.array_equal(got, ctx.verify_batch(crs, rows, proofs))
        assert np.array_equal(got, host_verdicts(key, rows, proofs))
        assert bool(got.all()) == all_good
        z = splitmix_z(rng, len(proofs))
        assert key.verify_batch_all(ctx, rows, proofs, z) == ctx.verify_batch_all(crs, rows, proofs, z) == all_good
        # the compressed call: the entries that have a compressed form (a proof off its curve or with a bad tag has none)
        pairs = []
        for r, p, v in zip(rows, proofs, got):
            try:
                pairs.append((r, zk.proof_compress(p), v))
            except zk.ZkError:
                assert not v
        c_rows, comp, want_c = np.stack([r for r, _, _ in pairs]), [c for _, c, _ in pairs], np.array([v for _, _, v in pairs])
        assert np.array_equal(key.verify_batch_compressed(ctx, c_rows, comp), want_c)
        assert np.array_equal(ctx.verify_batch_compressed(crs, c_rows, comp), want_c)
    assert len(honest) <= got.sum() < len(got) and len(pairs) >= 10
    # one bad proof among honest ones, first and last; the verdict is the CRS call's
    bad_at = int(np.flatnonzero(~got)[0])
    for at in (0, len(honest)):
        batch = honest[:at] + [t_proofs[bad_at]] + honest[at:]
        b_rows = np.concatenate([h_rows[:at], t_rows[bad_at][None], h_rows[at:]])
        z = splitmix_z(rng, len(batch))
        assert key.verify_batch_all(ctx, b_rows, batch, z) is False and ctx.verify_batch_all(crs, b_rows, batch, z) is False
    # z is applied exactly: each proof of a cancellation pair fails alone, the pair passes with z = (1, 1) only
    P1, P2 = _points(honest[0]), _points(honest[1])
    D = pyref.g1_mul(pyref.G1_GEN, 987654321)
    E = pyref.g1_mul(pyref.G1_GEN, 123456789)
    c_pair = [pyref.enc_proof(P1[0], P1[1], pyref.g1_add(P1[2], D)), pyref.enc_proof(P2[0], P2[1], pyref.g1_add(P2[2], pyref.g1_neg(D)))]
    a_pair = [pyref.enc_proof(pyref.g1_add(P1[0], E), P1[1], P1[2]), pyref.enc_proof(pyref.g1_add(P1[0], pyref.g1_neg(E)), P1[1], P1[2])]
    for pair in (c_pair, a_pair):
        assert not key.verify_batch(ctx, h_rows[:2], pair).any() and not host_verdicts(key, h_rows[:2], pair).any()
        assert key.verify_batch_all(ctx, h_rows[:2], pair, [1, 1]) is True and ctx.verify_batch_all(crs, h_rows[:2], pair, [1, 1]) is True
        assert key.verify_batch_all(ctx, h_rows[:2], pair, [1, 2]) is False


@pytest.mark.gpu
def test_statuses_are_the_crs_calls(ctx, simple):
    lib, crs, p = ctx.lib, simple["crs"], simple["proofs"]
    key = ctx.verifying_key(crs)
    pb = np.frombuffer(b"".join(p[:3]), dtype=np.uint8).copy()
    pp = pb.ctypes.data_as(_lib.u8p)
    ok = np.full(3, 7, np.int32)
    okp = ok.ctypes.data_as(C.POINTER(C.c_int))
    x = ints_to_limbs([2, 34, 2, R + 1, 2, 34])
    assert lib.zk_vk_verify_batch(ctx.ptr, key.ptr, x.ctypes.data_as(_lib.u64p), 2, pp, 3, okp) == _lib.ZK_ERR_RANGE
    assert (ok == 0).all() and "verify_batch: input >= r" in lib.zk_last_error(ctx.ptr).decode()
    good = ints_to_limbs([2, 34] * 3)
    gp = good.ctypes.data_as(_lib.u64p)
    for args in ((ctx.ptr, None, gp, 2, pp, 3, okp), (ctx.ptr, key.ptr, gp, 2, None, 3, okp), (ctx.ptr, key.ptr, gp, 2, pp, 3, None),
                 (ctx.ptr, key.ptr, None, 2, pp, 3, okp)):
        assert lib.zk_vk_verify_batch(*args) == _lib.ZK_ERR_ARG
        assert lib.zk_vk_verify_batch_compressed(*args) == _lib.ZK_ERR_ARG
    ok[:] = 7
    assert lib.zk_vk_verify_batch(ctx.ptr, key.ptr, gp, 2, pp, 0, okp) == _lib.ZK_OK and (ok == 7).all()
    for rows in ([[2]] * 4, [[2, 34, R + 5]] * 4, [[]] * 4, [[2, 25, 1]] * 4):       # truncation as zk_verify_batch
        assert np.array_equal(key.verify_batch(ctx, rows, p), ctx.verify_batch(crs, rows, p)), rows
        assert key.verify_batch_all(ctx, rows, p, [3, 5, 7, 9]) == ctx.verify_batch_all(crs, rows, p, [3, 5, 7, 9])
    one = C.c_int(7)
    z = np.array([[5, 0], [0, 0], [7, 0]], dtype=np.uint64)
    assert lib.zk_vk_verify_batch_all(ctx.ptr, key.ptr, gp, 2, pp, 3, z.ctypes.data_as(_lib.u64p), C.byref(one)) == _lib.ZK_ERR_ARG
    assert one.value == 0 and "z_j is 0" in lib.zk_last_error(ctx.ptr).decode()
    assert key.verify_batch_all(ctx, [], []) is True


@pytest.mark.gpu
def test_batch_larger_than_one_chunk(ctx, simple):
    key = ctx.verifying_key(simple["crs"])
    p = simple["proofs"][0]
    bad = bytearray(p); bad[100] ^= 4
    n = CHUNK + 1
    proofs = np.frombuffer(p, dtype=np.uint8)[None].repeat(n, axis=0)
    proofs[CHUNK] = np.frombuffer(bytes(bad), dtype=np.uint8)
    rows = ints_to_limbs([2, 34])[None].repeat(n, axis=0)
    want = np.ones(n, dtype=bool)
    want[CHUNK] = False
    assert np.array_equal(key.verify_batch(ctx, rows, proofs), want)
    sums = key.input_sums(ctx, rows[CHUNK - 1:])                    # two rows; and the sums over the chunk edge
    assert np.array_equal(key.input_sums(ctx, rows)[CHUNK - 1:], sums)


@pytest.mark.gpu
def test_transport_and_binding(ctx, simple):
    crs = simple["crs"]
    key = ctx.verifying_key(crs)
    rows, proofs = _tampered_batch(simple, 7)
    want = ctx.verify_batch(crs, rows, proofs)
    moved = zk.VerifyingKey.from_bytes(key.to_bytes())
    assert moved.to_bytes() == key.to_bytes()
    assert np.array_equal(moved.verify_batch(ctx, rows, proofs), want)
    assert np.array_equal(key.verify_batch(ctx, rows, proofs), want)
    other = zk.Context(0)
    try:
        with pytest.raises(zk.ZkError) as e:
            key.verify_batch(other, rows, proofs)                   # bound to `ctx`
        assert e.value.status == _lib.ZK_ERR_ARG
        with pytest.raises(zk.ZkError) as e:
            key.input_sums(other, [[2, 34]])
        assert e.value.status == _lib.ZK_ERR_ARG
        fresh = zk.VerifyingKey.from_bytes(key.to_bytes())          # an unbound copy binds to the second context
        assert np.array_equal(fresh.verify_batch(other, rows, proofs), want)
        with pytest.raises(zk.ZkError):
            fresh.verify_batch(ctx, rows, proofs)
    finally:
        other.close()
    assert host_verdicts(fresh, rows[:4], proofs[:4]).tolist() == want[:4].tolist()    # the host side outlives the context
    with pytest.raises(zk.ZkError) as e:
        fresh.verify_batch(ctx, rows, proofs)                       # its context is gone
    assert e.value.status == _lib.ZK_ERR_ARG
    fresh.close()
    assert np.array_equal(key.verify_batch(ctx, rows, proofs), want)


TEARDOWN = r"""
import sys
import numpy as np
import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs, SplitMix64
from zksnark_rs_amd.circuit import Circuit
order = sys.argv[1]
ctx = zk.Context(0)
c = Circuit(open(sys.argv[2]).read())
w = c.weights([3, 2, 4])
qap = c.qap(ctx)
rng = SplitMix64(31)
crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
proof = ctx.prove(crs, qap, w, rng.fr(), rng.fr())
key = ctx.verifying_key(crs)
assert key.verify_batch(ctx, [[2, 34]], [proof]).all()
assert key.input_sums(ctx, [[2, 34]]).any()
if order == "key_first":
    key.close()
    assert ctx.verify_batch(crs, [[2, 34]], [proof]).all()      # the context goes on working
    crs.close(); qap.close(); ctx.close()
else:
    crs.close(); qap.close(); ctx.close()
    assert key.verify([2, 34], proof)                           # the key goes on working on the host
    key.close()
print("done", order)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["key_first", "context_first"])
def test_key_and_context_go_in_either_order(order, tmp_path):
    script = tmp_path / "teardown.py"
    script.write_text(TEARDOWN)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, str(script), order, os.path.join(ZK_DIR, "simple.zk")], capture_output=True, text=True,
                         timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("done " + order)


@pytest.mark.gpu
def test_call_next_to_an_outstanding_proof(ctx, simple):
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    log_n = 12
    rng = SplitMix64(4245)
    m, l, u, v, w = chain_rows(log_n)
    weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    r, s = rng.fr(), rng.fr()
    want_proof = ctx.prove(crs, qap, weights, r, s)
    host = ctx.host_alloc(weights.shape)
    host[:] = weights
    rows, proofs = _tampered_batch(simple, 9)
    try:
        t = ctx.prove_submit_host(crs, qap, host.ctypes.data, weights.shape[0], r, s)
        key = ctx.verifying_key(simple["crs"])                       # from_crs, the binding and the table build under the ticket
        got = key.verify_batch(ctx, rows, proofs)
        key.close()                                                 # its buffers are retired, not freed, under the ticket
        proof = ctx.prove_wait(t)
    finally:
        ctx.host_free(host)
    assert proof == want_proof
    assert np.array_equal(got, ctx.verify_batch(simple["crs"], rows, proofs))
    assert ctx.verifying_key(crs).verify_batch(ctx, weights[None, 1:1 + l], [proof]).all()


@pytest.mark.gpu
def test_layers_agree(ctx, tmp_path):
    from zksnark_rs_amd import groth16
    code = open(os.path.join(ZK_DIR, "simple.zk")).read()
    qap = groth16.QAP.from_zk(ctx, code)
    w = groth16.weights(code, [3, 2, 4])
    sigma = groth16.setup(qap)
    proofs = [groth16.prove(qap, sigma, w) for _ in range(3)]
    rows = [[2, 34], [2, 25], [2, 34]]
    vk = groth16.verifying_key(sigma)
    assert groth16.verify_batch(vk, rows, proofs).tolist() == groth16.verify_batch(sigma, rows, proofs).tolist() == [True, False, True]
    assert [groth16.verify(vk, r, p) for r, p in zip(rows, proofs)] == [True, False, True]
    comp = [groth16.compress(p) for p in proofs]
    assert groth16.verify_batch_compressed(vk, rows, comp).tolist() == [True, False, True]
    assert groth16.verify_batch_all(vk, rows, proofs) is False and groth16.verify_batch_all(vk, [[2, 34]] * 3, proofs) is True
    restored = zk.VerifyingKey.from_bytes(vk.to_bytes())
    assert groth16.verify(restored, rows[0], proofs[0])
    with pytest.raises(ValueError):
        groth16.verify_batch(restored, rows, proofs)               # no context attached yet
    restored = zk.VerifyingKey.from_bytes(vk.to_bytes(), ctx=ctx)
    assert vk.ctx is ctx and restored.ctx is ctx
    assert groth16.verify_batch(restored, rows, proofs).tolist() == [True, False, True]
    # the C++ layer (include/zksnark.hpp)
    libdir = os.path.join(ROOT, "zksnark_rs_amd")
    exe = str(tmp_path / "vk_api")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "vk_api.cpp"),
                    "-o", exe, "-L", libdir, "-lzkgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([exe, os.path.join(ZK_DIR, "simple.zk"), str(tmp_path / "key.zkvk")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = dict(line.split(" ", 1) for line in res.stdout.strip().splitlines())
    assert lines["batch"] == lines["single"] == lines["crs"] == lines["compressed"] == lines["restored"] == "1 1 0 1 0 1"
    assert lines["all"] == "0" and lines["all_honest"] == "1" and lines["sums_equal"] == "1" and lines["other_context"] == "-1"
