// pairing.cpp -- host-only: the Fq2 / Fq6 / Fq12 tower, G2, the optimal ate Miller loop, the final exponentiation and the
// five C-ABI entries over them (include/halo2_hip.h: h2_pairing_check, h2_g2_mul_generator, h2_g2_mul, h2_g2_compress,
// h2_g2_decompress).  See pairing.hpp for the tower and DESIGN.md for the algorithm choices: affine Miller steps (one Fq2
// inversion each), a dense Fq12 product per line, the easy part of the final exponentiation by conjugation, inversion and
// the q^2 Frobenius, the hard part (q^4 - q^2 + 1) / r by plain square-and-multiply.  Every exponent is derived from the two
// moduli of field.hpp when the first entry runs; nothing here is tuned.
#include "pairing.hpp"

#include <string>
#include <vector>

#include "../../include/halo2_hip.h"

namespace h2 {
void set_last_error(const std::string& msg);

namespace pairing {
namespace {

typedef unsigned __int128 u128;
typedef std::vector<uint64_t> Big;  // little-endian limbs

Big big_from_u32(const uint32_t* l) {
    Big r(4);
    for (int i = 0; i < 4; i++) r[i] = (uint64_t)l[2 * i] | ((uint64_t)l[2 * i + 1] << 32);
    return r;
}
Big big_mul(const Big& a, const Big& b) {
    Big r(a.size() + b.size(), 0);
    for (size_t i = 0; i < a.size(); i++) {
        u128 c = 0;
        for (size_t j = 0; j < b.size(); j++) {
            c += (u128)a[i] * b[j] + r[i + j];
            r[i + j] = (uint64_t)c;
            c >>= 64;
        }
        r[i + b.size()] = (uint64_t)c;
    }
    return r;
}
int big_cmp(const Big& a, const Big& b) {  // any lengths
    const size_t n = a.size() > b.size() ? a.size() : b.size();
    for (size_t i = n; i-- > 0;) {
        const uint64_t x = i < a.size() ? a[i] : 0, y = i < b.size() ? b[i] : 0;
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}
void big_sub_in(Big& a, const Big& b) {  // a -= b, a >= b
    uint64_t borrow = 0;
    for (size_t i = 0; i < a.size(); i++) {
        const uint64_t y = i < b.size() ? b[i] : 0;
        const u128 t = (u128)a[i] - y - borrow;
        a[i] = (uint64_t)t;
        borrow = (uint64_t)(t >> 64) & 1;
    }
}
void big_add_small(Big& a, uint64_t v) {
    for (size_t i = 0; i < a.size() && v; i++) {
        const u128 t = (u128)a[i] + v;
        a[i] = (uint64_t)t;
        v = (uint64_t)(t >> 64);
    }
    if (v) a.push_back(v);
}
Big big_div(const Big& a, const Big& b) {  // floor(a / b) by binary long division (runs once, at initialisation)
    Big q(a.size(), 0), rem(b.size() + 1, 0);
    for (size_t bit = 64 * a.size(); bit-- > 0;) {
        for (size_t i = rem.size(); i-- > 0;) rem[i] = (rem[i] << 1) | (i ? rem[i - 1] >> 63 : 0);
        rem[0] |= (a[bit / 64] >> (bit % 64)) & 1;
        if (big_cmp(rem, b) >= 0) {
            big_sub_in(rem, b);
            q[bit / 64] |= (uint64_t)1 << (bit % 64);
        }
    }
    return q;
}
Big big_small(uint64_t v) { return Big(1, v); }
size_t big_bits(const Big& a) {
    for (size_t i = a.size(); i-- > 0;)
        if (a[i]) return 64 * i + 64 - (size_t)__builtin_clzll(a[i]);
    return 0;
}
bool big_bit(const Big& a, size_t i) { return (a[i / 64] >> (i % 64)) & 1; }

// ---- Fq -------------------------------------------------------------------------------------------------------------
Fq fq_zero() { return fp_zero<FqParams>(); }
Fq fq_one() { return fp_one<FqParams>(); }
Fq fq_small(uint64_t v) {
    Fq c = fq_zero();
    c.l[0] = (uint32_t)v;
    c.l[1] = (uint32_t)(v >> 32);
    return fp_to_mont(c);
}
Fq fq_pow(const Fq& a, const Big& e) {
    Fq acc = fq_one();
    for (size_t i = big_bits(e); i-- > 0;) {
        acc = fp_mul(acc, acc);
        if (big_bit(e, i)) acc = fp_mul(acc, a);
    }
    return acc;
}
bool limbs_below(const uint32_t* l, const uint32_t* mod) {  // l < mod as 256-bit integers
    for (int i = 7; i >= 0; i--)
        if (l[i] != mod[i]) return l[i] < mod[i];
    return false;
}
bool fq_load(const uint64_t* src, Fq& out) {  // 4 x u64 limbs (either representation) -> Fq; false when not below q
    for (int i = 0; i < 4; i++) {
        out.l[2 * i] = (uint32_t)src[i];
        out.l[2 * i + 1] = (uint32_t)(src[i] >> 32);
    }
    return limbs_below(out.l, FqParams::MOD);
}
void fq_store(const Fq& a, uint64_t* dst) {
    for (int i = 0; i < 4; i++) dst[i] = (uint64_t)a.l[2 * i] | ((uint64_t)a.l[2 * i + 1] << 32);
}

Fq2 fq2_zero() { return Fq2{fq_zero(), fq_zero()}; }
Fq2 fq2_one() { return Fq2{fq_one(), fq_zero()}; }
bool fq2_is_zero(const Fq2& a) { return fp_is_zero(a.c0) && fp_is_zero(a.c1); }
bool fq2_eq(const Fq2& a, const Fq2& b) { return fp_eq(a.c0, b.c0) && fp_eq(a.c1, b.c1); }
Fq2 fq2_dbl(const Fq2& a) { return Fq2{fp_dbl(a.c0), fp_dbl(a.c1)}; }
Fq2 fq2_conj(const Fq2& a) { return Fq2{a.c0, fp_neg(a.c1)}; }
Fq2 fq2_scale(const Fq2& a, const Fq& c) { return Fq2{fp_mul(a.c0, c), fp_mul(a.c1, c)}; }
Fq2 fq2_mul_xi(const Fq2& a) {  // (a0 + a1 u)(9 + u) = (9 a0 - a1) + (9 a1 + a0) u
    const Fq2 a8 = fq2_dbl(fq2_dbl(fq2_dbl(a)));
    const Fq2 a9 = fq2_add(a8, a);
    return Fq2{fp_sub(a9.c0, a.c1), fp_add(a9.c1, a.c0)};
}
Fq2 fq2_pow(const Fq2& a, const Big& e) {
    Fq2 acc = fq2_one();
    for (size_t i = big_bits(e); i-- > 0;) {
        acc = fq2_sqr(acc);
        if (big_bit(e, i)) acc = fq2_mul(acc, a);
    }
    return acc;
}

// ---- Fq6 ------------------------------------------------------------------------------------------------------------
Fq6 fq6_zero() { return Fq6{fq2_zero(), fq2_zero(), fq2_zero()}; }
Fq6 fq6_one() { return Fq6{fq2_one(), fq2_zero(), fq2_zero()}; }
Fq6 fq6_add(const Fq6& a, const Fq6& b) { return Fq6{fq2_add(a.a0, b.a0), fq2_add(a.a1, b.a1), fq2_add(a.a2, b.a2)}; }
Fq6 fq6_sub(const Fq6& a, const Fq6& b) { return Fq6{fq2_sub(a.a0, b.a0), fq2_sub(a.a1, b.a1), fq2_sub(a.a2, b.a2)}; }
Fq6 fq6_neg(const Fq6& a) { return Fq6{fq2_neg(a.a0), fq2_neg(a.a1), fq2_neg(a.a2)}; }
Fq6 fq6_mul_v(const Fq6& a) { return Fq6{fq2_mul_xi(a.a2), a.a0, a.a1}; }  // v^3 = xi
Fq6 fq6_mul(const Fq6& a, const Fq6& b) {
    // Karatsuba over the three coefficients: 6 Fq2 products
    const Fq2 t0 = fq2_mul(a.a0, b.a0), t1 = fq2_mul(a.a1, b.a1), t2 = fq2_mul(a.a2, b.a2);
    const Fq2 s12 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.a1, a.a2), fq2_add(b.a1, b.a2)), t1), t2);  // a1 b2 + a2 b1
    const Fq2 s01 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.a0, a.a1), fq2_add(b.a0, b.a1)), t0), t1);  // a0 b1 + a1 b0
    const Fq2 s02 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.a0, a.a2), fq2_add(b.a0, b.a2)), t0), t2);  // a0 b2 + a2 b0
    return Fq6{fq2_add(t0, fq2_mul_xi(s12)), fq2_add(s01, fq2_mul_xi(t2)), fq2_add(s02, t1)};
}
Fq6 fq6_inv(const Fq6& a) {
    const Fq2 t0 = fq2_sub(fq2_sqr(a.a0), fq2_mul_xi(fq2_mul(a.a1, a.a2)));
    const Fq2 t1 = fq2_sub(fq2_mul_xi(fq2_sqr(a.a2)), fq2_mul(a.a0, a.a1));
    const Fq2 t2 = fq2_sub(fq2_sqr(a.a1), fq2_mul(a.a0, a.a2));
    const Fq2 d = fq2_add(fq2_mul(a.a0, t0), fq2_mul_xi(fq2_add(fq2_mul(a.a2, t1), fq2_mul(a.a1, t2))));
    const Fq2 di = fq2_inv(d);
    return Fq6{fq2_mul(t0, di), fq2_mul(t1, di), fq2_mul(t2, di)};
}

// ---- Fq12 -----------------------------------------------------------------------------------------------------------
Fq12 fq12_conj(const Fq12& a) { return Fq12{a.c0, fq6_neg(a.c1)}; }  // a^(q^6)
// the coefficient of w^i, i < 6, of c0 + c1 w with w^2 = v
Fq2* fq12_coeff(Fq12& a, int i) {
    Fq6& h = (i & 1) ? a.c1 : a.c0;
    return i / 2 == 0 ? &h.a0 : (i / 2 == 1 ? &h.a1 : &h.a2);
}
Fq12 fq12_pow(const Fq12& a, const Big& e) {
    Fq12 acc = fq12_one();
    for (size_t i = big_bits(e); i-- > 0;) {
        acc = fq12_mul(acc, acc);
        if (big_bit(e, i)) acc = fq12_mul(acc, a);
    }
    return acc;
}

struct Consts {
    Big q, r, qp1_4, hard;
    Fq half, three;
    Fq2 b2;                 // 3 / xi
    Fq2 frob_x, frob_y;     // xi^((q-1)/3), xi^((q-1)/2): the q-power Frobenius on twist coordinates
    Fq2 frob2_w[6];         // (xi^((q^2-1)/6))^i: the q^2-power Frobenius on the coefficient of w^i
    G2Affine gen;
    uint64_t loop_lo;       // 6u + 2 = 2^64 + loop_lo
};

Fq fq_from_dec(const char* s) {  // decimal -> Montgomery (the generator's published coordinates)
    Fq acc = fq_zero();
    const Fq ten = fq_small(10);
    for (; *s; s++) acc = fp_add(fp_mul(acc, ten), fq_small((uint64_t)(*s - '0')));
    return acc;
}

const Consts& consts() {
    static const Consts C = [] {
        Consts c;
        c.q = big_from_u32(FqParams::MOD);
        c.r = big_from_u32(FrParams::MOD);
        Big t = c.q;
        big_add_small(t, 1);
        c.qp1_4 = big_div(t, big_small(4));
        Big qm1 = c.q;
        big_sub_in(qm1, big_small(1));
        const Big q2 = big_mul(c.q, c.q);
        Big q2m1 = q2;
        big_sub_in(q2m1, big_small(1));
        Big h = big_mul(q2, q2);  // q^4 - q^2 + 1
        big_sub_in(h, q2);
        big_add_small(h, 1);
        c.hard = big_div(h, c.r);
        c.half = fp_inv(fq_small(2));
        c.three = fq_small(3);
        const Fq2 xi = Fq2{fq_small(9), fq_one()};
        c.b2 = fq2_scale(fq2_inv(xi), c.three);
        c.frob_x = fq2_pow(xi, big_div(qm1, big_small(3)));
        c.frob_y = fq2_pow(xi, big_div(qm1, big_small(2)));
        const Fq2 g = fq2_pow(xi, big_div(q2m1, big_small(6)));
        c.frob2_w[0] = fq2_one();
        for (int i = 1; i < 6; i++) c.frob2_w[i] = fq2_mul(c.frob2_w[i - 1], g);
        c.gen.inf = false;
        c.gen.x = Fq2{fq_from_dec("10857046999023057135944570762232829481370756359578518086990519993285655852781"),
                      fq_from_dec("11559732032986387107991004021392285783925812861821192530917403151452391805634")};
        c.gen.y = Fq2{fq_from_dec("8495653923123431417604973247489272438418190587263600148770280649306958101930"),
                      fq_from_dec("4082367875863433681332203403145435568316851327593401208105741076214120093531")};
        const u128 loop = (u128)6 * 4965661367192848881ull + 2;  // 6u + 2, 65 bits
        c.loop_lo = (uint64_t)loop;
        return c;
    }();
    return C;
}

Fq12 fq12_frob2(const Fq12& a) {
    Fq12 r = a;
    const Consts& C = consts();
    for (int i = 1; i < 6; i++) {
        Fq2* c = fq12_coeff(r, i);
        *c = fq2_mul(*c, C.frob2_w[i]);
    }
    return r;
}

G2Affine g2_frobenius(const G2Affine& p) {
    const Consts& C = consts();
    return G2Affine{fq2_mul(fq2_conj(p.x), C.frob_x), fq2_mul(fq2_conj(p.y), C.frob_y), p.inf};
}

// the line through the untwisted T with slope lambda w, at P:  yP - lambda xP w + (lambda xT - yT) w^3
Fq12 line_value(const Fq2& lambda, const G2Affine& t, const G1Affine& p) {
    Fq12 l{fq6_zero(), fq6_zero()};
    l.c0.a0 = Fq2{p.y, fq_zero()};
    *fq12_coeff(l, 1) = fq2_neg(fq2_scale(lambda, p.x));
    *fq12_coeff(l, 3) = fq2_sub(fq2_mul(lambda, t.x), t.y);
    return l;
}
// the vertical through T at P: xP - xT w^2
Fq12 vertical_value(const G2Affine& t, const G1Affine& p) {
    Fq12 l{fq6_zero(), fq6_zero()};
    l.c0.a0 = Fq2{p.x, fq_zero()};
    *fq12_coeff(l, 2) = fq2_neg(t.x);
    return l;
}
// f *= l_{T,T}(P), T = 2T
void double_step(Fq12& f, G2Affine& t, const G1Affine& p) {
    if (t.inf) return;
    if (fq2_is_zero(t.y)) {  // a point of order two: not in the subgroup, kept total all the same
        f = fq12_mul(f, vertical_value(t, p));
        t.inf = true;
        return;
    }
    const Fq2 x2 = fq2_sqr(t.x);
    const Fq2 lambda = fq2_mul(fq2_add(fq2_dbl(x2), x2), fq2_inv(fq2_dbl(t.y)));
    f = fq12_mul(f, line_value(lambda, t, p));
    const Fq2 x3 = fq2_sub(fq2_sqr(lambda), fq2_dbl(t.x));
    t.y = fq2_sub(fq2_mul(lambda, fq2_sub(t.x, x3)), t.y);
    t.x = x3;
}
// f *= l_{T,Q}(P), T = T + Q
void add_step(Fq12& f, G2Affine& t, const G2Affine& q, const G1Affine& p) {
    if (t.inf) {
        t = q;
        return;
    }
    if (fq2_eq(t.x, q.x)) {
        if (fq2_eq(t.y, q.y)) {
            double_step(f, t, p);
        } else {
            f = fq12_mul(f, vertical_value(t, p));
            t.inf = true;
        }
        return;
    }
    const Fq2 lambda = fq2_mul(fq2_sub(q.y, t.y), fq2_inv(fq2_sub(q.x, t.x)));
    f = fq12_mul(f, line_value(lambda, t, p));
    const Fq2 x3 = fq2_sub(fq2_sub(fq2_sqr(lambda), t.x), q.x);
    t.y = fq2_sub(fq2_mul(lambda, fq2_sub(t.x, x3)), t.y);
    t.x = x3;
}

}  // namespace

// ---- Fq2 (public) ---------------------------------------------------------------------------------------------------
Fq2 fq2_add(const Fq2& a, const Fq2& b) { return Fq2{fp_add(a.c0, b.c0), fp_add(a.c1, b.c1)}; }
Fq2 fq2_sub(const Fq2& a, const Fq2& b) { return Fq2{fp_sub(a.c0, b.c0), fp_sub(a.c1, b.c1)}; }
Fq2 fq2_neg(const Fq2& a) { return Fq2{fp_neg(a.c0), fp_neg(a.c1)}; }
Fq2 fq2_mul(const Fq2& a, const Fq2& b) {
    const Fq t0 = fp_mul(a.c0, b.c0), t1 = fp_mul(a.c1, b.c1);
    const Fq m = fp_mul(fp_add(a.c0, a.c1), fp_add(b.c0, b.c1));
    return Fq2{fp_sub(t0, t1), fp_sub(fp_sub(m, t0), t1)};
}
Fq2 fq2_sqr(const Fq2& a) {
    const Fq m = fp_mul(a.c0, a.c1);
    return Fq2{fp_mul(fp_add(a.c0, a.c1), fp_sub(a.c0, a.c1)), fp_dbl(m)};
}
Fq2 fq2_inv(const Fq2& a) {  // 0 -> 0
    const Fq d = fp_inv(fp_add(fp_mul(a.c0, a.c0), fp_mul(a.c1, a.c1)));
    return Fq2{fp_mul(a.c0, d), fp_neg(fp_mul(a.c1, d))};
}
// q = 3 mod 4: Fq roots are a^((q+1)/4); an Fq2 root from the norm (the "complex method")
bool fq2_sqrt(const Fq2& a, Fq2& out) {
    const Consts& C = consts();
    auto fq_sqrt = [&](const Fq& v, Fq& root) {
        root = fq_pow(v, C.qp1_4);
        return fp_eq(fp_mul(root, root), v);
    };
    Fq s;
    if (fp_is_zero(a.c1)) {
        if (fq_sqrt(a.c0, s)) {
            out = Fq2{s, fq_zero()};
            return true;
        }
        if (fq_sqrt(fp_neg(a.c0), s)) {  // -1 is a non-residue: (s u)^2 = -s^2 = a0
            out = Fq2{fq_zero(), s};
            return true;
        }
        return false;
    }
    Fq n;
    if (!fq_sqrt(fp_add(fp_mul(a.c0, a.c0), fp_mul(a.c1, a.c1)), n)) return false;
    Fq x0;
    if (!fq_sqrt(fp_mul(fp_add(a.c0, n), C.half), x0) && !fq_sqrt(fp_mul(fp_sub(a.c0, n), C.half), x0)) return false;
    const Fq x1 = fp_mul(a.c1, fp_inv(fp_dbl(x0)));
    out = Fq2{x0, x1};
    return fq2_eq(fq2_sqr(out), a);
}

// ---- Fq12 (public) --------------------------------------------------------------------------------------------------
Fq12 fq12_one() { return Fq12{fq6_one(), fq6_zero()}; }
Fq12 fq12_mul(const Fq12& a, const Fq12& b) {
    const Fq6 t0 = fq6_mul(a.c0, b.c0), t1 = fq6_mul(a.c1, b.c1);
    const Fq6 m = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(b.c0, b.c1));
    return Fq12{fq6_add(t0, fq6_mul_v(t1)), fq6_sub(fq6_sub(m, t0), t1)};
}
Fq12 fq12_inv(const Fq12& a) {  // (c0 - c1 w) / (c0^2 - v c1^2)
    const Fq6 d = fq6_inv(fq6_sub(fq6_mul(a.c0, a.c0), fq6_mul_v(fq6_mul(a.c1, a.c1))));
    return Fq12{fq6_mul(a.c0, d), fq6_neg(fq6_mul(a.c1, d))};
}
bool fq12_is_one(const Fq12& a) {
    return fq2_eq(a.c0.a0, fq2_one()) && fq2_is_zero(a.c0.a1) && fq2_is_zero(a.c0.a2) && fq2_is_zero(a.c1.a0) &&
           fq2_is_zero(a.c1.a1) && fq2_is_zero(a.c1.a2);
}

// ---- G2 -------------------------------------------------------------------------------------------------------------
G2Affine g2_generator() { return consts().gen; }
bool g2_on_curve(const G2Affine& p) {
    if (p.inf) return true;
    return fq2_eq(fq2_sqr(p.y), fq2_add(fq2_mul(fq2_sqr(p.x), p.x), consts().b2));
}
G2Jac g2_double(const G2Jac& p) {  // a = 0 (dbl-2009-l)
    if (fq2_is_zero(p.z)) return p;
    const Fq2 A = fq2_sqr(p.x), B = fq2_sqr(p.y), Cc = fq2_sqr(B);
    const Fq2 D = fq2_dbl(fq2_sub(fq2_sub(fq2_sqr(fq2_add(p.x, B)), A), Cc));
    const Fq2 E = fq2_add(fq2_dbl(A), A), F = fq2_sqr(E);
    G2Jac r;
    r.x = fq2_sub(F, fq2_dbl(D));
    r.y = fq2_sub(fq2_mul(E, fq2_sub(D, r.x)), fq2_dbl(fq2_dbl(fq2_dbl(Cc))));
    r.z = fq2_dbl(fq2_mul(p.y, p.z));
    return r;
}
G2Jac g2_add_mixed(const G2Jac& p, const G2Affine& q) {
    if (q.inf) return p;
    if (fq2_is_zero(p.z)) return G2Jac{q.x, q.y, fq2_one()};
    const Fq2 z2 = fq2_sqr(p.z);
    const Fq2 u2 = fq2_mul(q.x, z2), s2 = fq2_mul(fq2_mul(q.y, p.z), z2);
    const Fq2 h = fq2_sub(u2, p.x), rr = fq2_sub(s2, p.y);
    if (fq2_is_zero(h)) {
        if (fq2_is_zero(rr)) return g2_double(p);
        return G2Jac{fq2_one(), fq2_one(), fq2_zero()};
    }
    const Fq2 hh = fq2_sqr(h), hhh = fq2_mul(h, hh), v = fq2_mul(p.x, hh);
    G2Jac r;
    r.x = fq2_sub(fq2_sub(fq2_sqr(rr), hhh), fq2_dbl(v));
    r.y = fq2_sub(fq2_mul(rr, fq2_sub(v, r.x)), fq2_mul(p.y, hhh));
    r.z = fq2_mul(p.z, h);
    return r;
}
G2Affine g2_to_affine(const G2Jac& p) {
    if (fq2_is_zero(p.z)) return G2Affine{fq2_zero(), fq2_zero(), true};
    const Fq2 zi = fq2_inv(p.z), zi2 = fq2_sqr(zi);
    return G2Affine{fq2_mul(p.x, zi2), fq2_mul(fq2_mul(p.y, zi2), zi), false};
}
G2Affine g2_add_affine(const G2Affine& p, const G2Affine& q) {
    if (p.inf) return q;
    return g2_to_affine(g2_add_mixed(G2Jac{p.x, p.y, fq2_one()}, q));
}
static G2Jac g2_mul_jac(const G2Affine& p, const uint64_t* scalar, size_t limbs) {
    G2Jac acc{fq2_one(), fq2_one(), fq2_zero()};
    if (p.inf) return acc;
    for (size_t i = 64 * limbs; i-- > 0;) {
        acc = g2_double(acc);
        if ((scalar[i / 64] >> (i % 64)) & 1) acc = g2_add_mixed(acc, p);
    }
    return acc;
}
G2Affine g2_mul(const G2Affine& p, const uint64_t scalar[4]) { return g2_to_affine(g2_mul_jac(p, scalar, 4)); }
bool g2_in_subgroup(const G2Affine& p) {
    if (p.inf) return true;
    const Big& r = consts().r;
    return fq2_is_zero(g2_mul_jac(p, r.data(), 4).z);
}

// ---- the pairing ----------------------------------------------------------------------------------------------------
Fq12 miller_loop(const G1Affine* p, const G2Affine* q, size_t pairs) {
    const Consts& C = consts();
    std::vector<G1Affine> ps;
    std::vector<G2Affine> qs, ts;
    for (size_t i = 0; i < pairs; i++)
        if (!p[i].inf && !q[i].inf) {
            ps.push_back(p[i]);
            qs.push_back(q[i]);
        }
    ts = qs;  // bit 64 of 6u + 2
    Fq12 f = fq12_one();
    for (int bit = 63; bit >= 0; bit--) {
        f = fq12_mul(f, f);
        for (size_t i = 0; i < ps.size(); i++) {
            double_step(f, ts[i], ps[i]);
            if ((C.loop_lo >> bit) & 1) add_step(f, ts[i], qs[i], ps[i]);
        }
    }
    for (size_t i = 0; i < ps.size(); i++) {
        const G2Affine q1 = g2_frobenius(qs[i]);
        G2Affine nq2 = g2_frobenius(q1);
        nq2.y = fq2_neg(nq2.y);
        add_step(f, ts[i], q1, ps[i]);
        add_step(f, ts[i], nq2, ps[i]);
    }
    return f;
}
Fq12 final_exponentiation(const Fq12& f) {
    const Fq12 a = fq12_mul(fq12_conj(f), fq12_inv(f));  // f^(q^6 - 1)
    const Fq12 b = fq12_mul(fq12_frob2(a), a);            // ^(q^2 + 1)
    return fq12_pow(b, consts().hard);                    // ^((q^4 - q^2 + 1) / r)
}
bool pairing_check(const G1Affine* p, const G2Affine* q, size_t pairs) {
    return fq12_is_one(final_exponentiation(miller_loop(p, q, pairs)));
}

// ---- the C ABI's encodings ------------------------------------------------------------------------------------------
namespace {
int invalid(const char* msg) {
    set_last_error(msg);
    return H2_ERR_INVALID;
}
bool all_zero(const uint64_t* p, size_t n) {
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) o |= p[i];
    return o == 0;
}
// 64 B affine Montgomery, identity (0,0); false: a coordinate is not below q, or the point is not on y^2 = x^3 + 3
bool g1_read(const uint64_t* xy, G1Affine& out) {
    if (!fq_load(xy, out.x) || !fq_load(xy + 4, out.y)) return false;
    out.inf = all_zero(xy, 8);
    if (out.inf) return true;
    const Fq rhs = fp_add(fp_mul(fp_mul(out.x, out.x), out.x), consts().three);
    return fp_eq(fp_mul(out.y, out.y), rhs);
}
// 128 B affine Montgomery x.c0 x.c1 y.c0 y.c1, identity all zeros; 0 = fine, else the reason
const char* g2_read(const uint64_t* xy, G2Affine& out, bool subgroup) {
    if (!fq_load(xy, out.x.c0) || !fq_load(xy + 4, out.x.c1) || !fq_load(xy + 8, out.y.c0) || !fq_load(xy + 12, out.y.c1))
        return "a G2 coordinate is not a canonical residue";
    out.inf = all_zero(xy, 16);
    if (out.inf) return nullptr;
    if (!g2_on_curve(out)) return "a G2 point is not on the curve";
    if (subgroup && !g2_in_subgroup(out)) return "a G2 point is outside the order-r subgroup";
    return nullptr;
}
void g2_write(const G2Affine& p, uint64_t* xy) {
    if (p.inf) {
        for (int i = 0; i < 16; i++) xy[i] = 0;
        return;
    }
    fq_store(p.x.c0, xy);
    fq_store(p.x.c1, xy + 4);
    fq_store(p.y.c0, xy + 8);
    fq_store(p.y.c1, xy + 12);
}
// the sign bit of the 64-byte encoding: the parity of the canonical y.c0, of y.c1 when y.c0 == 0 (y and -y always differ in it)
uint32_t g2_y_sign(const Fq2& y) {
    const Fq c0 = fp_from_mont(y.c0);
    if (!fp_is_zero(c0)) return c0.l[0] & 1;
    return fp_from_mont(y.c1).l[0] & 1;
}
}  // namespace

}  // namespace pairing
}  // namespace h2

using namespace h2;
using namespace h2::pairing;

extern "C" {

int h2_pairing_check(const uint64_t* g1_xy, const uint64_t* g2_xy, size_t pairs, int* ok) {
    if (!ok || (pairs && (!g1_xy || !g2_xy))) return invalid("h2_pairing_check: null argument");
    *ok = 0;
    std::vector<G1Affine> ps(pairs);
    std::vector<G2Affine> qs(pairs);
    for (size_t i = 0; i < pairs; i++) {
        if (!g1_read(g1_xy + 8 * i, ps[i])) return invalid("h2_pairing_check: a G1 point is not canonical or not on the curve");
        if (const char* why = g2_read(g2_xy + 16 * i, qs[i], true)) return invalid(why);
    }
    *ok = pairing_check(ps.data(), qs.data(), pairs) ? 1 : 0;
    return H2_OK;
}

int h2_g2_mul_generator(const uint64_t scalar[4], uint64_t out_xy[16]) {
    if (!scalar || !out_xy) return invalid("h2_g2_mul_generator: null argument");
    Fq probe;  // (only the limb split is used)
    fq_load(scalar, probe);
    if (!limbs_below(probe.l, FrParams::MOD)) return invalid("h2_g2_mul_generator: the scalar is not below r");
    g2_write(g2_mul(g2_generator(), scalar), out_xy);
    return H2_OK;
}

int h2_g2_mul(const uint64_t xy[16], const uint64_t scalar[4], uint64_t out_xy[16]) {
    if (!xy || !scalar || !out_xy) return invalid("h2_g2_mul: null argument");
    Fq probe;  // (only the limb split is used)
    fq_load(scalar, probe);
    if (!limbs_below(probe.l, FrParams::MOD)) return invalid("h2_g2_mul: the scalar is not below r");
    G2Affine p;
    if (const char* why = g2_read(xy, p, true)) return invalid(why);
    g2_write(g2_mul(p, scalar), out_xy);
    return H2_OK;
}

int h2_g2_compress(const uint64_t xy[16], uint8_t out[64]) {
    if (!xy || !out) return invalid("h2_g2_compress: null argument");
    G2Affine p;
    if (const char* why = g2_read(xy, p, false)) return invalid(why);
    for (int i = 0; i < 64; i++) out[i] = 0;
    if (p.inf) return H2_OK;
    const Fq c[2] = {fp_from_mont(p.x.c0), fp_from_mont(p.x.c1)};
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 32; i++) out[32 * j + i] = (uint8_t)(c[j].l[i / 4] >> (8 * (i % 4)));
    out[63] |= (uint8_t)(g2_y_sign(p.y) << 7);
    return H2_OK;
}

int h2_g2_decompress(const uint8_t in[64], uint64_t out_xy[16]) {
    if (!in || !out_xy) return invalid("h2_g2_decompress: null argument");
    const uint32_t sign = in[63] >> 7;
    Fq c[2];
    bool zero = true;
    for (int j = 0; j < 2; j++) {
        c[j] = fp_zero<FqParams>();
        for (int i = 0; i < 32; i++) {
            const uint8_t b = (j == 1 && i == 31) ? (uint8_t)(in[63] & 0x7f) : in[32 * j + i];
            c[j].l[i / 4] |= (uint32_t)b << (8 * (i % 4));
            zero = zero && b == 0;
        }
        if (!limbs_below(c[j].l, FqParams::MOD)) return invalid("h2_g2_decompress: x is not a canonical residue");
    }
    if (zero) {
        if (sign) return invalid("h2_g2_decompress: the identity with a sign bit");
        g2_write(G2Affine{Fq2{c[0], c[0]}, Fq2{c[0], c[0]}, true}, out_xy);
        return H2_OK;
    }
    G2Affine p;
    p.inf = false;
    p.x = Fq2{fp_to_mont(c[0]), fp_to_mont(c[1])};
    const Fq2 rhs = fq2_add(fq2_mul(fq2_sqr(p.x), p.x), consts().b2);
    if (!fq2_sqrt(rhs, p.y)) return invalid("h2_g2_decompress: x^3 + b has no square root");
    if (g2_y_sign(p.y) != sign) p.y = fq2_neg(p.y);
    if (!g2_in_subgroup(p)) return invalid("h2_g2_decompress: the point is outside the order-r subgroup");
    g2_write(p, out_xy);
    return H2_OK;
}

}  // extern "C"
