// point_codec.cuh -- the compressed proof form (128 bytes: A 32 | B 64 | C 32, include/zkgpu.h "Compressed proof bytes") for
// host and device (ZK_HD): square roots in Fq and Fq2, the canonical sign of y, the point encoders and decoders, and the two
// whole-proof conversions.  zk_proof_compress / zk_proof_decompress run these routines on the host, the kernels of
// proof_codec.hip run the same ones one point per lane.
//
// A compressed block is the big-endian x coordinate with a flag in the two top bits of its first byte (q < 2^254 leaves them
// free): 10 = finite, y is the smaller of {y, q - y}; 11 = finite, y is the larger; 01 = infinity, every other bit zero;
// 00 = never valid.  G2 blocks are x.c1 | x.c0 (EIP-197 order, as in the 259-byte form) with the flag in x.c1's first byte and
// the two top bits of x.c0's first byte zero.
//
// THE SIGN IS TAKEN ON THE CANONICAL INTEGER, never on the Montgomery residue: "larger" means the integer y in [0, q) is
// > (q - 1) / 2 (G2: the same test on y.c1 unless y.c1 == 0, then on y.c0).  Elements live in Montgomery form here (y R mod q),
// and the residue of y being above (q - 1) / 2 says nothing about y itself, so fq_is_larger converts first.
//
// Decompression checks the encoding and curve membership only.  The order-r subgroup test of B stays in dec_g2 (pairing.cuh),
// behind every verify call: a 128-byte string may carry a twist point outside G2 exactly as a 259-byte one may.
#pragma once
#include "pairing.cuh"

namespace zk {

struct FqWords {
    uint32_t w[8];
};
constexpr FqWords fq_modulus_shr(int s) {   // q >> s, 0 < s < 32
    FqWords e{};
    for (int i = 0; i < 8; ++i) e.w[i] = (FqParams::P[i] >> s) | (i + 1 < 8 ? FqParams::P[i + 1] << (32 - s) : 0u);
    return e;
}
static_assert((FqParams::P[0] & 3u) == 3u, "the square root below needs q = 3 mod 4");
static constexpr FqWords FQ_QM3_4 = fq_modulus_shr(2);   // (q - 3) / 4, 252 bits
static constexpr FqWords FQ_HALF = fq_modulus_shr(1);    // (q - 1) / 2

// a^((q - 3) / 4) by a fixed chain: a 4-bit window over the constant exponent, 14 multiplications for the table, then
// 62 x (4 squarings + 1 multiplication), the same sequence for every a (a zero digit multiplies by one).  The table is indexed
// by the exponent's digits, which every lane of a wave shares.  One body per translation unit.
static ZK_NI Fq fq_pow_qm3_4(const Fq& a) {
    Fq tab[16];
    tab[0] = Fq::one();
    tab[1] = a;
    for (int i = 2; i < 16; ++i) tab[i] = tab[i - 1] * a;
    Fq acc = tab[(FQ_QM3_4.w[7] >> 24) & 15];   // digit 62, the top one
#pragma unroll 1
    for (int k = 61; k >= 0; --k) {
        acc = acc.sqr().sqr().sqr().sqr();
        acc = acc * tab[(FQ_QM3_4.w[k >> 3] >> ((k & 7) * 4)) & 15];
    }
    return acc;
}
// root = a^((q + 1) / 4) = a * a^((q - 3) / 4); accepted iff root^2 == a (q = 3 mod 4).  rinv = a^((q - 3) / 4) is 1 / root
// whenever a is a non-zero square: root * rinv = a^((q - 1) / 2) = 1.
ZK_HD bool fq_sqrt_inv(const Fq& a, Fq& root, Fq& rinv) {
    rinv = fq_pow_qm3_4(a);
    root = rinv * a;
    return root.sqr() == a;
}
ZK_HD bool fq_sqrt(const Fq& a, Fq& root) {
    Fq rinv;
    return fq_sqrt_inv(a, root, rinv);
}
// The complex method (i^2 = -1), three exponentiations whatever a is; no branch before the selects at the end.
//   a.c1 == 0: a.c0 or -a.c0 is a square (-1 is not): root = (sqrt a.c0, 0) or (0, sqrt -a.c0); c = a.c0^((q + 1) / 4) is the
//              root of whichever it is, so c^2 == a.c0 decides.
//   otherwise: s = sqrt(a.c0^2 + a.c1^2) (the norm; no root: a is not a square), d = (a.c0 + s) / 2 or (a.c0 - s) / 2, whichever
//              is a square (their product is -a.c1^2 / 4, a non-square, so exactly one is), x0 = sqrt d, x1 = a.c1 / (2 x0) with
//              1 / x0 from the same exponentiation.
// Whatever the branch, the result is accepted only if root^2 == a.
ZK_HD bool fq2_sqrt(const Fq2& a, Fq2& root) {
    const bool real = a.c1.is_zero();
    Fq s;
    fq_sqrt(a.c0.sqr() + a.c1.sqr(), s);
    const Fq d1 = fq_half(a.c0 + s), d2 = fq_half(a.c0 - s);
    const Fq in1 = real ? a.c0 : d1;
    Fq r1, i1, r2, i2;
    const bool sq1 = fq_sqrt_inv(in1, r1, i1);
    fq_sqrt_inv(d2, r2, i2);
    const Fq x0 = sq1 ? r1 : r2;
    const Fq x1 = a.c1 * fq_half(sq1 ? i1 : i2);
    const Fq2 general{x0, x1};
    const Fq2 special{sq1 ? r1 : Fq::zero(), sq1 ? Fq::zero() : r1};
    root = real ? special : general;
    return root.sqr() == a;
}

// true iff the canonical integer of y (Montgomery in) is > (q - 1) / 2
ZK_HD bool fq_is_larger(const Fq& y) {
    const Fq c = y.to_canonical();
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = (uint64_t)FQ_HALF.w[i] - c.l[i] - br;
        br = (uint32_t)(t >> 63);
    }
    return br != 0;
}
ZK_HD bool fq2_is_larger(const Fq2& y) { return y.c1.is_zero() ? fq_is_larger(y.c0) : fq_is_larger(y.c1); }

// 32 big-endian bytes <-> limbs; `first_mask` clears the flag bits of the first byte
ZK_HD Fq fq_raw_from_be(const uint8_t* be, uint8_t first_mask) {
    Fq x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint8_t b0 = i == 0 ? (uint8_t)(be[0] & first_mask) : be[4 * i];
        x.l[7 - i] = ((uint32_t)b0 << 24) | ((uint32_t)be[4 * i + 1] << 16) | ((uint32_t)be[4 * i + 2] << 8) | be[4 * i + 3];
    }
    return x;
}
ZK_HD void fq_to_be(const Fq& x_mont, uint8_t* out) {
    const Fq x = x_mont.to_canonical();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t w = x.l[7 - i];
        out[4 * i + 0] = (uint8_t)(w >> 24);
        out[4 * i + 1] = (uint8_t)(w >> 16);
        out[4 * i + 2] = (uint8_t)(w >> 8);
        out[4 * i + 3] = (uint8_t)w;
    }
}
ZK_HD void fill_bytes(uint8_t* p, size_t n, uint8_t v) {
    for (size_t i = 0; i < n; ++i) p[i] = v;
}

// ---- compressed blocks -> points.  Every path runs the same exponentiations; validity is a select at the end. ----
// One byte string per point: x < q, x^3 + b a square.  y = 0 cannot occur (both curve orders are odd, so there is no
// 2-torsion); if it ever did, only flag 10 would be accepted.
ZK_HD bool dec_g1c(const uint8_t* p, G1A& out) {
    const unsigned flag = p[0] >> 6;
    uint8_t rest = p[0] & 0x3f;
    for (int i = 1; i < 32; ++i) rest |= p[i];
    const Fq xr = fq_raw_from_be(p, 0x3f);
    const bool in_range = xr.raw_in_range();
    const Fq x = Fq::from_canonical(xr);
    Fq y;
    const bool sq = fq_sqrt(x.sqr() * x + fq_small(3), y);
    const bool want_larger = flag == 3;
    const Fq ysel = fq_is_larger(y) == want_larger ? y : -y;
    const bool finite = flag >= 2 && in_range && sq && !(y.is_zero() && want_larger);
    out = finite ? G1A{x, ysel} : G1A::infinity();
    return finite || (flag == 1 && rest == 0);
}
ZK_HD bool dec_g2c(const uint8_t* p, G2A& out) {
    const unsigned flag = p[0] >> 6;
    uint8_t rest = p[0] & 0x3f;
    for (int i = 1; i < 64; ++i) rest |= p[i];
    const Fq2 xr{fq_raw_from_be(p + 32, 0xff), fq_raw_from_be(p, 0x3f)};   // x.c1 | x.c0
    const bool in_range = xr.raw_in_range() && (p[32] >> 6) == 0;
    const Fq2 x = Fq2::from_canonical(xr);
    Fq2 y;
    const bool sq = fq2_sqrt(x.sqr() * x + fq2_from_words(TWIST_B), y);
    const bool want_larger = flag == 3;
    const Fq2 ysel = fq2_is_larger(y) == want_larger ? y : -y;
    const bool finite = flag >= 2 && in_range && sq && !(y.is_zero() && want_larger);
    out = finite ? G2A{x, ysel} : G2A::infinity();
    return finite || (flag == 1 && rest == 0);
}

// ---- points -> compressed blocks ----
ZK_HD void enc_g1c(const G1A& a, uint8_t* out) {
    if (a.is_inf()) {
        fill_bytes(out, 32, 0);
        out[0] = 0x40;
        return;
    }
    fq_to_be(a.x, out);
    out[0] |= fq_is_larger(a.y) ? 0xc0 : 0x80;
}
ZK_HD void enc_g2c(const G2A& a, uint8_t* out) {
    if (a.is_inf()) {
        fill_bytes(out, 64, 0);
        out[0] = 0x40;
        return;
    }
    fq_to_be(a.x.c1, out);
    fq_to_be(a.x.c0, out + 32);
    out[0] |= fq2_is_larger(a.y) ? 0xc0 : 0x80;
}

// ---- the 65 / 129 byte blocks of the 259-byte form ----
ZK_HD void enc_g1u(const G1A& a, uint8_t* out) {
    if (a.is_inf()) {
        fill_bytes(out, 65, 0);
        return;
    }
    out[0] = 4;
    fq_to_be(a.x, out + 1);
    fq_to_be(a.y, out + 33);
}
ZK_HD void enc_g2u(const G2A& a, uint8_t* out) {
    if (a.is_inf()) {
        fill_bytes(out, 129, 0);
        return;
    }
    out[0] = 4;
    fq_to_be(a.x.c1, out + 1);
    fq_to_be(a.x.c0, out + 33);
    fq_to_be(a.y.c1, out + 65);
    fq_to_be(a.y.c0, out + 97);
}
// dec_g2 without [r]Q == infinity: tag, range and the twist's equation only (dec_g1 already is that reader for G1)
ZK_HD bool dec_g2_curve(const uint8_t* p, G2A& out) {
    out = G2A::infinity();
    if (p[0] == 0) return all_zero(p + 1, 128);
    if (p[0] != 4) return false;
    const Fq2 xr{fq_raw_from_be(p + 33, 0xff), fq_raw_from_be(p + 1, 0xff)}, yr{fq_raw_from_be(p + 97, 0xff), fq_raw_from_be(p + 65, 0xff)};
    if (!xr.raw_in_range() || !yr.raw_in_range()) return false;
    const G2A q{Fq2::from_canonical(xr), Fq2::from_canonical(yr)};
    if (q.is_inf() || !(q.y.sqr() == q.x.sqr() * q.x + fq2_from_words(TWIST_B))) return false;
    out = q;
    return true;
}

// ---- one block of a proof: 32 -> 65 and 64 -> 129 bytes.  A block that does not decode is written as 0xFF bytes: tag 0xFF is
// refused by every decoder of the 259-byte form (zero bytes would read as infinity). ----
ZK_HD bool decompress_g1_block(const uint8_t* in, uint8_t* out) {
    G1A a;
    const bool ok = dec_g1c(in, a);
    if (ok) enc_g1u(a, out);
    else fill_bytes(out, 65, 0xff);
    return ok;
}
ZK_HD bool decompress_g2_block(const uint8_t* in, uint8_t* out) {
    G2A a;
    const bool ok = dec_g2c(in, a);
    if (ok) enc_g2u(a, out);
    else fill_bytes(out, 129, 0xff);
    return ok;
}

// ---- whole proofs ----
// 128 -> 259 bytes; false and 259 x 0xFF unless all three blocks are valid encodings of points on their curves
ZK_HD bool proof_decompress(const uint8_t* in, uint8_t* out) {
    const bool a = decompress_g1_block(in, out), b = decompress_g2_block(in + 32, out + 65), c = decompress_g1_block(in + 96, out + 194);
    if (!(a && b && c)) fill_bytes(out, 259, 0xff);
    return a && b && c;
}
// 259 -> 128 bytes; false and 128 zero bytes (flag 00) unless every block has a legal tag, coordinates < q and lies on its curve.
// No square roots and no subgroup test.
ZK_HD bool proof_compress(const uint8_t* in, uint8_t* out) {
    G1A a, c;
    G2A b;
    if (!(dec_g1(in, a) && dec_g2_curve(in + 65, b) && dec_g1(in + 194, c))) {
        fill_bytes(out, 128, 0);
        return false;
    }
    enc_g1c(a, out);
    enc_g2c(b, out + 32);
    enc_g1c(c, out + 96);
    return true;
}

}  // namespace zk
