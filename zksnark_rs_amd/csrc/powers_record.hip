// powers_record.hip -- the record of a powers-of-tau contribution: three of crs_contribution.hip's Schnorr records, one per
// secret (s on tau_g1[1], a on alpha_tau_g1[0], b on beta_tau_g1[0]), each bound to its own role tag
//   tag_role = SHA-256("ZKPOWv1\0" | role byte 1 / 2 / 3 | tag)
// so that a record proves nothing in another role.  Host code, no context and no device (as crs_contribution.hip); the sanitizer
// program of tests/test_powers_recode_host.py compiles it alone.
#include "crs_contribution.hpp"
#include "sha256.hpp"

namespace zk {

void powers_role_tag(int role, const uint8_t tag[32], uint8_t out[32]) {
    static const uint8_t zero_tag[32] = {0};
    const uint8_t rb = (uint8_t)role;
    Sha256 h;
    h.update("ZKPOWv1", 8);   // with its terminating zero
    h.update(&rb, 1);
    h.update(tag ? tag : zero_tag, 32);
    h.finish(out);
}

namespace {
Fr pw_words(const uint64_t* w) {
    Fr x;
    for (int i = 0; i < 4; ++i) { x.l[2 * i] = (uint32_t)w[i]; x.l[2 * i + 1] = (uint32_t)(w[i] >> 32); }
    return x;
}
}  // namespace

// 0 = made; otherwise the status.  secrets: s, a, b canonical; nonces: three canonical scalars or null (OS)
int powers_contribution_prove(const uint64_t before[24], const uint64_t secrets[12], const uint64_t* nonces, const uint8_t tag[32],
                              zk_powers_contribution* out) {
    Fr v[3], k[3];
    int status = ZK_OK;
    for (int i = 0; i < 3 && status == ZK_OK; ++i) {
        v[i] = pw_words(secrets + 4 * i);
        if (!v[i].raw_in_range()) status = ZK_ERR_RANGE;
        else if (v[i].is_zero()) status = ZK_ERR_DIV_BY_ZERO;
        if (nonces) {
            k[i] = pw_words(nonces + 4 * i);
            if (status == ZK_OK && !k[i].raw_in_range()) status = ZK_ERR_RANGE;
        } else {
            k[i] = draw_scalar_nonzero();
        }
    }
    zk_powers_contribution rec;
    zk_crs_contribution* part[3] = {&rec.tau, &rec.alpha, &rec.beta};
    for (int i = 0; i < 3 && status == ZK_OK; ++i) {
        uint8_t role_tag[32];
        powers_role_tag(i + 1, tag, role_tag);
        uint64_t any = 0;
        for (int w = 0; w < 8; ++w) any |= before[8 * i + w];
        if (!any) { std::memset(part[i], 0, sizeof(zk_crs_contribution)); continue; }   // an infinity before-point (a degenerate transcript): no proof exists, the part stays zero and never verifies
        if (!contribution_prove(before + 8 * i, v[i], k[i], role_tag, part[i])) status = ZK_ERR_RANGE;
    }
    wipe(v, sizeof(v));
    wipe(k, sizeof(k));
    if (status == ZK_OK) *out = rec;
    return status;
}

bool powers_contribution_verify(const zk_powers_contribution& c, const uint8_t tag[32]) {
    const zk_crs_contribution* part[3] = {&c.tau, &c.alpha, &c.beta};
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
        uint8_t role_tag[32];
        powers_role_tag(i + 1, tag, role_tag);
        ok = contribution_verify(*part[i], role_tag) && ok;
    }
    return ok;
}

}  // namespace zk

extern "C" {

int zk_powers_contribution_prove(const uint64_t before[24], const uint64_t secrets[12], const uint64_t nonces[12], const uint8_t tag[32],
                                 zk_powers_contribution* out) {
    if (!before || !secrets || !out) return ZK_ERR_ARG;
    return zk::powers_contribution_prove(before, secrets, nonces, tag, out);
}

int zk_powers_contribution_verify(const zk_powers_contribution* c, const uint8_t tag[32], int* ok) {
    if (!c || !ok) return ZK_ERR_ARG;
    *ok = zk::powers_contribution_verify(*c, tag) ? 1 : 0;
    return ZK_OK;
}

}  // extern "C"
