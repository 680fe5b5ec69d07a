// pairing.hpp -- the BN254 optimal ate pairing and G2 on the HOST: what a verifier needs after its MSMs
// (poly/multiopen.rs:29-55 `Decider`, plonk/verifier.rs:496-507: e(left, [s]G2) * e(-right, G2) == 1) and what
// Params::unsafe_setup / ParamsVerifier carry of G2 (poly/commitment.rs:113-116, :33-40).  The reference takes all of
// this from the un-vendored pairing_bn256 crate.
//
// Tower over the host Fq of field.hpp (Montgomery form throughout):
//   Fq2  = Fq[u]  / (u^2 + 1)
//   Fq6  = Fq2[v] / (v^3 - xi),  xi = 9 + u
//   Fq12 = Fq6[w] / (w^2 - v)            (w^6 = xi)
// G2 lives on the sextic D-twist y^2 = x^3 + 3 / xi over Fq2 and maps into E(Fq12) by (x, y) -> (x w^2, y w^3).
// No device code: a pairing is one serial chain of Fq products.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "field.hpp"

namespace h2 {
namespace pairing {

struct Fq2 {
    Fq c0, c1;
};
struct Fq6 {
    Fq2 a0, a1, a2;
};
struct Fq12 {
    Fq6 c0, c1;
};
struct G2Affine {  // identity: inf (the ABI encodes it as all zeros)
    Fq2 x, y;
    bool inf;
};
struct G2Jac {     // identity: z == 0
    Fq2 x, y, z;
};
struct G1Affine {
    Fq x, y;
    bool inf;
};

Fq2 fq2_add(const Fq2& a, const Fq2& b);
Fq2 fq2_sub(const Fq2& a, const Fq2& b);
Fq2 fq2_neg(const Fq2& a);
Fq2 fq2_mul(const Fq2& a, const Fq2& b);
Fq2 fq2_sqr(const Fq2& a);
Fq2 fq2_inv(const Fq2& a);
bool fq2_sqrt(const Fq2& a, Fq2& out);
Fq12 fq12_one();
Fq12 fq12_mul(const Fq12& a, const Fq12& b);
Fq12 fq12_inv(const Fq12& a);
bool fq12_is_one(const Fq12& a);

G2Affine g2_generator();
bool g2_on_curve(const G2Affine& p);
bool g2_in_subgroup(const G2Affine& p);  // [r] p == identity
G2Jac g2_double(const G2Jac& p);
G2Jac g2_add_mixed(const G2Jac& p, const G2Affine& q);
G2Affine g2_add_affine(const G2Affine& p, const G2Affine& q);
G2Affine g2_to_affine(const G2Jac& p);
G2Affine g2_mul(const G2Affine& p, const uint64_t scalar[4]);  // scalar: plain little-endian integer

// product of the Miller loops f_{6u+2,Q}(P) l_{[6u+2]Q,pi(Q)}(P) l_{[6u+2]Q+pi(Q),-pi^2(Q)}(P) over all pairs (identities skipped)
Fq12 miller_loop(const G1Affine* p, const G2Affine* q, size_t pairs);
Fq12 final_exponentiation(const Fq12& f);
bool pairing_check(const G1Affine* p, const G2Affine* q, size_t pairs);  // prod e(p_i, q_i) == 1, one final exponentiation

}  // namespace pairing
}  // namespace h2
