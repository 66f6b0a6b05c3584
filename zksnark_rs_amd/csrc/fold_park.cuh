// fold_park.cuh -- the G2 fold's running sum with three of its four coordinates parked in LDS (add_xyzz_from_parked), in a header of
// its own so that a test program can call it without the kernels and explicit instantiations of msm_impl.hpp.
#pragma once
#include "lazy29.cuh"

namespace zk {

// Workgroup size of the reduction tail (merge / fold / weigh).  ONE wave: while an accumulation fills the chip, a 256-lane
// workgroup of a 150..250-register kernel needs all four SIMDs of a CU to have room at the same moment, which only happens in
// the accumulation's last round (the timeline showed the previous proof's G2 tail still running 8 ms after its accumulation
// and the next proof's sort waiting behind it on the same stream); a single wave fits wherever one accumulation wave retires.
constexpr int TAIL_THREADS = 64;

// G2 folds with Y, ZZ and ZZZ of the running sum in LDS between their uses.  The general addition over Fq2 holds 233 registers at
// once; capped at the tail kernels' 168 the by-value form (add_xyzz) spilled 700 B per lane -- 1.9 GB of scratch traffic per proof of
// 2^20 gates, a ninth of everything a proof moved -- and the coordinate-by-coordinate form (add_xyzz_from, ZK_FOLD_PARK=0) still 53
// dwords per addition (0.7 GB).  Parked: 15 KB of LDS per workgroup, 20 ds_read_b128 + 15 ds_write_b128 per addition, no scratch on
// the path of an ordinary addition.  Same box, 5 x 20 steps interleaved: by value 102.53, by coordinate 103.76, parked 103.49,
// by value at 2 waves per SIMD (233 registers, ZK_FOLD_G2_WAVES=2) 103.06 proofs/s; HBM bytes per proof 17.51 / 16.41 / 15.70 /
// 15.62 GB (profiles/r5_experiments.txt item 14).
#ifndef ZK_FOLD_PARK
#define ZK_FOLD_PARK 1
#endif
struct FoldPark { int4 r[3][5][TAIL_THREADS]; };   // [Y | ZZ | ZZZ][row][lane]
__device__ __forceinline__ void fpark_put(FoldPark* pk, int which, const Fp2R<FqParams>& v) {
    int4* row = &pk->r[which][0][threadIdx.x];
    row[0 * TAIL_THREADS] = make_int4(v.c0.v[0], v.c0.v[1], v.c0.v[2], v.c0.v[3]);
    row[1 * TAIL_THREADS] = make_int4(v.c0.v[4], v.c0.v[5], v.c0.v[6], v.c0.v[7]);
    row[2 * TAIL_THREADS] = make_int4(v.c0.v[8], v.c1.v[0], v.c1.v[1], v.c1.v[2]);
    row[3 * TAIL_THREADS] = make_int4(v.c1.v[3], v.c1.v[4], v.c1.v[5], v.c1.v[6]);
    row[4 * TAIL_THREADS] = make_int4(v.c1.v[7], v.c1.v[8], 0, 0);
}
__device__ __forceinline__ Fp2R<FqParams> fpark_get(const FoldPark* pk, int which) {
    asm volatile("" ::: "memory");   // a fresh read every time: the point is NOT to keep the value in registers
    const int4* row = &pk->r[which][0][threadIdx.x];
    const int4 a = row[0 * TAIL_THREADS], b = row[1 * TAIL_THREADS], c = row[2 * TAIL_THREADS], d = row[3 * TAIL_THREADS], e = row[4 * TAIL_THREADS];
    Fp2R<FqParams> v;
    v.c0.v[0] = a.x; v.c0.v[1] = a.y; v.c0.v[2] = a.z; v.c0.v[3] = a.w; v.c0.v[4] = b.x; v.c0.v[5] = b.y; v.c0.v[6] = b.z; v.c0.v[7] = b.w;
    v.c0.v[8] = c.x; v.c1.v[0] = c.y; v.c1.v[1] = c.z; v.c1.v[2] = c.w; v.c1.v[3] = d.x; v.c1.v[4] = d.y; v.c1.v[5] = d.z; v.c1.v[6] = d.w;
    v.c1.v[7] = e.x; v.c1.v[8] = e.y;
    return v;
}
// add_xyzz_from (lazy29.cuh) with the sum's Y / ZZ / ZZZ in LDS: same formulas, same order, same bounds
__device__ __forceinline__ void add_xyzz_from_parked(Fp2R<FqParams>& X, bool& inf, FoldPark* pk, const XyzzR<Fp2R<FqParams>>* q) {
    typedef Fp2R<FqParams> L;
    if (q->inf) return;
    if (inf) {
        X = q->X; fpark_put(pk, 0, q->Y); fpark_put(pk, 1, q->ZZ); fpark_put(pk, 2, q->ZZZ);
        inf = false;
        return;
    }
    L U1, P;
    {
        const L qzz = q->ZZ;
        U1 = X * qzz;
    }
    asm volatile("" ::: "memory");
    {
        const L qx = q->X;
        P = qx * fpark_get(pk, 1) - U1;
    }
    asm volatile("" ::: "memory");
    const L PP = P.sqr();
    if (PP.is_zero_mod_p()) {
        const L qy = q->Y;
        const bool same = (qy * fpark_get(pk, 2) - fpark_get(pk, 0) * q->ZZZ).sqr().is_zero_mod_p();
        if (same) {
            XyzzR<L> t = *q;
            dbl_xyzz(t);
            X = t.X; fpark_put(pk, 0, t.Y); fpark_put(pk, 1, t.ZZ); fpark_put(pk, 2, t.ZZZ);
        } else inf = true;
        return;
    }
    {
        const L qzz = q->ZZ;
        fpark_put(pk, 1, (fpark_get(pk, 1) * qzz) * PP);
    }
    asm volatile("" ::: "memory");
    const L Q = U1 * PP;
    const L PPP = P * PP;
    L S1, R;
    {
        const L qzzz = q->ZZZ;
        S1 = fpark_get(pk, 0) * qzzz;
        const L Z3 = fpark_get(pk, 2);
        const L T = Z3 * qzzz;
        asm volatile("" ::: "memory");
        const L qy = q->Y;
        R = qy * Z3 - S1;
        fpark_put(pk, 2, T * PPP);
    }
    asm volatile("" ::: "memory");
    const L X3 = (R.sqr() - PPP - (Q + Q)).norm();
    fpark_put(pk, 0, xyzz_ydiff(R, Q - X3, S1, PPP));
    X = X3;
}

}  // namespace zk
