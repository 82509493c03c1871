// The fields of ncg_field_check (include/ncg.h): one row per field id, read by the C ABI (api.hip: validity and buffer sizes),
// the device launcher (selfcheck.hip, which pairs every row with its kernel) and the host twin (hosttest.hip
// ht_field_check_shape).  A new field is one row here, one launcher row in selfcheck.hip and one shared check function.
#pragma once

namespace ncg {

struct SelfCheckField {
  int field;       // the id of ncg_field_check
  int wa, wb, wo;  // 32-bit words per row of a, b and out
  int lanes;       // lanes per row (2: the lane-paired Fp2 form); the four-lane ops of fields 12 / 13 take four rows' worth
};

inline constexpr SelfCheckField SELFCHECK_FIELDS[] = {
    {0, 9, 9, 8, 1},         // fe9.hpp over secp256k1 p: raw limbs -> canonical wire words (fe9_check.hpp)
    {1, 9, 9, 8, 1},         //   ... over ed25519 p
    {2, 12, 12, 12, 1},      // bls12-381 Fe29 from and to canonical wire words
    {3, 28, 28, 12, 1},      // Fe29 raw limbs [a, c], [b, d]
    {4, 56, 56, 24, 2},      // lane-paired Fp2 raw limbs [a, c], [b, d], every element c0 then c1
    {5, 18, 18, 9, 1},       // fused Fe9 expressions over secp256k1 p: [a, c], [b, d] -> 9 raw limbs (fe9_check.hpp)
    {6, 18, 18, 9, 1},       //   ... over ed25519 p
    {7, 27, 18, 27, 1},      // secp256k1 ladder pieces (secp_ladder_check.hpp)
    {8, 9, 9, 9, 1},         // fr29 raw limbs (fr29_check.hpp)
    {9, 9, 9, 9, 1},         // bn254 Fe9 Montgomery raw limbs (fe9m_check.hpp)
    {10, 36, 36, 36, 1},     // the MSM groups (group_check.hpp), one stored accumulator of 4 FW words each: secp256k1
    {11, 36, 36, 36, 1},     //   ed25519
    {12, 56, 56, 56, 1},     //   bls12-381 G1
    {13, 112, 112, 112, 2},  //   lane-paired G2
    {14, 36, 36, 36, 1},     //   bn254 G1
    // 15 is unassigned and refused
    {16, 36, 9, 36, 1},      // X25519 ladder pieces (x25519.hpp)
    {17, 36, 9, 36, 1},      // ristretto255 pieces (ristretto.hpp)
};
constexpr int SELFCHECK_NFIELDS = (int)(sizeof(SELFCHECK_FIELDS) / sizeof(SELFCHECK_FIELDS[0]));

// the row of `field`, or null for an id that is not registered
constexpr const SelfCheckField* selfcheck_field(int field) {
  for (int i = 0; i < SELFCHECK_NFIELDS; i++)
    if (SELFCHECK_FIELDS[i].field == field) return &SELFCHECK_FIELDS[i];
  return nullptr;
}

}  // namespace ncg
