// crs_contribution.hpp -- what crs_contribution.hip (host code: the scalar's preparation, the record) and crs_contribute.hip (the
// kernel, the CRS side) share.
#pragma once
#include "common.hpp"

namespace zk {

// One scalar k < r prepared for k_g1_scale: k = k1 + k2 lambda (gbasis.hip's GLV split restated for the host, rounding to nearest),
// each half as a width-4 non-adjacent form with the half's sign folded in: digit i of half h is 0 or odd in [-7, 7],
// sum_i d_h[i] 2^i = k_h, no two non-zero digits of a half within four positions.  |k_h| < 2^128 gives at most 129 digits; SC_DIGITS
// leaves a margin that scalar_recode checks instead of assuming.  top = the highest position with a non-zero digit in either half, -1 for k = 0.
constexpr int SC_DIGITS = 132;
struct ScaleDigits {
    int8_t d1[SC_DIGITS], d2[SC_DIGITS];
    int32_t top;
};
// |k1|, |k2| as five 32-bit words each and their signs
void glv_split_host(const uint32_t k[8], uint32_t k1[5], bool& neg1, uint32_t k2[5], bool& neg2);
void scalar_recode(const uint32_t k[8], ScaleDigits& out);
void wipe(void* p, size_t bytes);   // zeroes memory in a way the optimiser keeps

// z G for the record's Schnorr proof and its check: host code over ec.cuh
bool contribution_prove(const uint64_t delta_before[8], const Fr& d_can, const Fr& nonce_can, const uint8_t tag[32], zk_crs_contribution* out);
bool contribution_verify(const zk_crs_contribution& c, const uint8_t tag[32]);
Fr draw_scalar_nonzero();   // 256 bits from the OS reduced mod r, never 0 (canonical)

// powers_record.hip: the three records of a powers-of-tau contribution under their role tags (host code)
void powers_role_tag(int role, const uint8_t tag[32], uint8_t out[32]);
int powers_contribution_prove(const uint64_t before[24], const uint64_t secrets[12], const uint64_t* nonces, const uint8_t tag[32],
                              zk_powers_contribution* out);   // a status; *out untouched unless ZK_OK
bool powers_contribution_verify(const zk_powers_contribution&, const uint8_t tag[32]);

}  // namespace zk
