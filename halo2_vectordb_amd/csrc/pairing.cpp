// Host arithmetic of the Verify arm (include/vdb.h b7): the BN254 optimal ate pairing and the G2 group law.  Not a hot path — a
// proof costs two Miller loops and one final exponentiation — so plain 4 x 64-bit Montgomery arithmetic, no GPU, no vdb_init.
// Public standard, restated from the definition:
//   Fq2  = Fq[u] / (u^2 + 1);  the twist E': y^2 = x^3 + 3 / xi over Fq2, xi = 9 + u;
//   Fq12 = Fq[w] / (w^12 - 18 w^6 + 82), so w^6 = xi and an Fq2 element a + b u sits in Fq12 as (a - 9 b) + b w^6;
//   the untwisting map (x, y) -> (x w^2, y w^3) puts E' into E(Fq12), y^2 = x^3 + 3;
//   Frobenius on E': (x, y) -> (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2)), since w^q = w xi^((q-1)/6);
//   Miller loop over 6 x + 2 (x = 4965661367192848881) from the top bit, then the lines through pi(Q) and -pi^2(Q);
//   final exponentiation f^((q^12 - 1) / r).
// Lines are evaluated at P on E(Fq12) with the slope taken on the twist (lambda w is the slope of the untwisted points):
//   through T1, T2 (tangent when equal): -y_P + (lambda x_P) w + (y_1 - lambda x_1) w^3;  vertical: x_P - x_1 w^2.
#include <stdint.h>
#include <string.h>

#include "../../include/vdb.h"

namespace vdb {
void set_error(const char* fmt, ...);   // core.hip
}

namespace {

typedef unsigned __int128 u128;

struct Mod {
  uint64_t p[4], r2[4], one[4], inv;
};
const Mod MQ = {{0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
                {0xf32cfc5b538afa89ull, 0xb5e71911d44501fbull, 0x47ab1eff0a417ff6ull, 0x06d89f71cab8351full},
                {0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full},
                0x87d20782e4866389ull};
const Mod MR = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
                {0x1bb8e645ae216da7ull, 0x53fe3ab1e35c59e3ull, 0x8c49833d53bb8085ull, 0x0216d0b17f4e44a5ull},
                {0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full},
                0xc2e1f593efffffffull};
// (q^12 - 1) / r, 2790 bits, little-endian limbs
const uint64_t FINAL_EXP[44] = {
    0x86964b64ca86f120ull, 0x40a4efb7e54523a4ull, 0x837fa97896e84abbull, 0x361102b6b9b2b918ull,
    0xc0de81def35692daull, 0xbe04c7e8a6c3c760ull, 0xd766f9c9d570bb7full, 0xc230974d83561841ull,
    0x5bba1668c3be69a3ull, 0x7f3811c410526294ull, 0x29baee7ddadda71cull, 0xbf813b8d145da900ull,
    0x641bbadf423f9a2cull, 0xa80bb4ea44eacc5eull, 0xcd65664814fde37cull, 0x4a0364b9580291d2ull,
    0xee93dfb10826f0ddull, 0x6b42db8dc5514724ull, 0xbb10cf430b0f3785ull, 0x40494e406f804216ull,
    0x55cfe107acf3aafbull, 0x2088ec80e0ebae87ull, 0x846a3ed011a337a0ull, 0x48a45a4a1e3a5195ull,
    0xe5664568dfc50e16ull, 0xab6a41294c0cc4ebull, 0x82d0d602d268c7daull, 0x6668449aed3cc48aull,
    0x5062cd0fb2015dfcull, 0x7f2940a8b1ddb3d1ull, 0x77f5b63a2a226448ull, 0xfef0781361e443aeull,
    0xf977870e88d5c6c8ull, 0x790364a61f676baaull, 0x5887e72eceaddea3ull, 0x1377e563a09a1b70ull,
    0x0c54efee1bd8c3b2ull, 0x3ec3d15ad524d8f7ull, 0xdaf15466b2383a5dull, 0xe1e30a73bb94fec0ull,
    0x6a1c71015f3f7be2ull, 0x842d43bf6369b1ffull, 0x20fddadf107d20bcull, 0x0000002f4b6dc970ull,
};

struct F {
  uint64_t v[4];
};
struct F2 {
  F a, b;  // a + b u
};
struct F12 {
  F c[12];  // sum c[i] w^i
};
struct G2 {
  F2 x, y;
  bool inf;
};

bool f_is_zero(const F& a) { return (a.v[0] | a.v[1] | a.v[2] | a.v[3]) == 0; }
bool f_eq(const F& a, const F& b) { return memcmp(a.v, b.v, 32) == 0; }
bool lt_p(const uint64_t* a, const uint64_t* p) {
  for (int i = 3; i >= 0; i--)
    if (a[i] != p[i]) return a[i] < p[i];
  return false;
}
F f_sub_p(F a, const Mod& m) {   // a - p when a >= p
  if (lt_p(a.v, m.p)) return a;
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    u128 d = (u128)a.v[i] - m.p[i] - br;
    a.v[i] = (uint64_t)d;
    br = (uint64_t)(d >> 64) & 1;
  }
  return a;
}
// Montgomery product a b / 2^256 (CIOS); inputs below p < 2^254, so the result is below 2p before the last subtraction
F mmul(const F& a, const F& b, const Mod& m) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    uint64_t C = 0;
    for (int j = 0; j < 4; j++) {
      u128 s = (u128)a.v[j] * b.v[i] + t[j] + C;
      t[j] = (uint64_t)s;
      C = (uint64_t)(s >> 64);
    }
    u128 s = (u128)t[4] + C;
    t[4] = (uint64_t)s;
    t[5] = (uint64_t)(s >> 64);
    const uint64_t mm = t[0] * m.inv;
    s = (u128)mm * m.p[0] + t[0];
    C = (uint64_t)(s >> 64);
    for (int j = 1; j < 4; j++) {
      s = (u128)mm * m.p[j] + t[j] + C;
      t[j - 1] = (uint64_t)s;
      C = (uint64_t)(s >> 64);
    }
    s = (u128)t[4] + C;
    t[3] = (uint64_t)s;
    t[4] = t[5] + (uint64_t)(s >> 64);
  }
  F r = {{t[0], t[1], t[2], t[3]}};
  return f_sub_p(r, m);
}
F fq_mul(const F& a, const F& b) { return mmul(a, b, MQ); }
F fq_add(const F& a, const F& b) {
  F r;
  uint64_t c = 0;
  for (int i = 0; i < 4; i++) {
    u128 s = (u128)a.v[i] + b.v[i] + c;
    r.v[i] = (uint64_t)s;
    c = (uint64_t)(s >> 64);
  }
  return f_sub_p(r, MQ);
}
F fq_sub(const F& a, const F& b) {
  F r;
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    u128 d = (u128)a.v[i] - b.v[i] - br;
    r.v[i] = (uint64_t)d;
    br = (uint64_t)(d >> 64) & 1;
  }
  if (br) {
    uint64_t c = 0;
    for (int i = 0; i < 4; i++) {
      u128 s = (u128)r.v[i] + MQ.p[i] + c;
      r.v[i] = (uint64_t)s;
      c = (uint64_t)(s >> 64);
    }
  }
  return r;
}
F fq_zero() { return F{{0, 0, 0, 0}}; }
F fq_one() { return F{{MQ.one[0], MQ.one[1], MQ.one[2], MQ.one[3]}}; }
F fq_neg(const F& a) { return fq_sub(fq_zero(), a); }
F fq_canon(const uint64_t* v) { return mmul(F{{v[0], v[1], v[2], v[3]}}, F{{MQ.r2[0], MQ.r2[1], MQ.r2[2], MQ.r2[3]}}, MQ); }
F fq_small(uint64_t v) {
  const uint64_t w[4] = {v, 0, 0, 0};
  return fq_canon(w);
}
// a^e, e little-endian limbs
F fq_pow(const F& a, const uint64_t* e, int limbs) {
  F acc = fq_one();
  for (int i = 64 * limbs - 1; i >= 0; i--) {
    acc = fq_mul(acc, acc);
    if ((e[i / 64] >> (i % 64)) & 1) acc = fq_mul(acc, a);
  }
  return acc;
}
const uint64_t Q_MINUS_2[4] = {0x3c208c16d87cfd45ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
const uint64_t Q_MINUS_1_OVER_3[4] = {0x69602eb24829a9c2ull, 0xdd2b2385cd7b4384ull, 0xe81ac1e7808072c9ull, 0x10216f7ba065e00dull};
const uint64_t Q_MINUS_1_OVER_2[4] = {0x9e10460b6c3e7ea3ull, 0xcbc0b548b438e546ull, 0xdc2822db40c0ac2eull, 0x183227397098d014ull};
F fq_inv(const F& a) { return fq_pow(a, Q_MINUS_2, 4); }   // 0 -> 0

F2 f2_add(const F2& x, const F2& y) { return F2{fq_add(x.a, y.a), fq_add(x.b, y.b)}; }
F2 f2_sub(const F2& x, const F2& y) { return F2{fq_sub(x.a, y.a), fq_sub(x.b, y.b)}; }
F2 f2_neg(const F2& x) { return F2{fq_neg(x.a), fq_neg(x.b)}; }
F2 f2_conj(const F2& x) { return F2{x.a, fq_neg(x.b)}; }
F2 f2_mul(const F2& x, const F2& y) {
  return F2{fq_sub(fq_mul(x.a, y.a), fq_mul(x.b, y.b)), fq_add(fq_mul(x.a, y.b), fq_mul(x.b, y.a))};
}
F2 f2_scale(const F2& x, const F& s) { return F2{fq_mul(x.a, s), fq_mul(x.b, s)}; }
F2 f2_inv(const F2& x) {
  const F t = fq_inv(fq_add(fq_mul(x.a, x.a), fq_mul(x.b, x.b)));
  return F2{fq_mul(x.a, t), fq_neg(fq_mul(x.b, t))};
}
bool f2_is_zero(const F2& x) { return f_is_zero(x.a) && f_is_zero(x.b); }
bool f2_eq(const F2& x, const F2& y) { return f_eq(x.a, y.a) && f_eq(x.b, y.b); }
F2 f2_pow(const F2& x, const uint64_t* e, int limbs) {
  F2 acc = F2{fq_one(), fq_zero()};
  for (int i = 64 * limbs - 1; i >= 0; i--) {
    acc = f2_mul(acc, acc);
    if ((e[i / 64] >> (i % 64)) & 1) acc = f2_mul(acc, x);
  }
  return acc;
}

F12 f12_one() {
  F12 r;
  for (int i = 0; i < 12; i++) r.c[i] = fq_zero();
  r.c[0] = fq_one();
  return r;
}
F12 f12_mul(const F12& x, const F12& y) {
  static const F C18 = fq_small(18), C82 = fq_small(82);
  F t[23];
  for (int i = 0; i < 23; i++) t[i] = fq_zero();
  for (int i = 0; i < 12; i++) {
    if (f_is_zero(x.c[i])) continue;
    for (int j = 0; j < 12; j++) t[i + j] = fq_add(t[i + j], fq_mul(x.c[i], y.c[j]));
  }
  for (int e = 22; e >= 12; e--) {     // w^12 = 18 w^6 - 82
    t[e - 6] = fq_add(t[e - 6], fq_mul(C18, t[e]));
    t[e - 12] = fq_sub(t[e - 12], fq_mul(C82, t[e]));
  }
  F12 r;
  for (int i = 0; i < 12; i++) r.c[i] = t[i];
  return r;
}
bool f12_is_one(const F12& x) {
  const F12 o = f12_one();
  for (int i = 0; i < 12; i++)
    if (!f_eq(x.c[i], o.c[i])) return false;
  return true;
}
// x += v w^k for an Fq2 element v = a + b u = (a - 9 b) + b w^6 (k < 6)
void f12_put(F12& x, const F2& v, int k) {
  static const F C9 = fq_small(9);
  x.c[k] = fq_add(x.c[k], fq_sub(v.a, fq_mul(C9, v.b)));
  x.c[k + 6] = fq_add(x.c[k + 6], v.b);
}

struct Consts {
  F2 b2, gamma2, gamma3;   // 3 / xi, xi^((q-1)/3), xi^((q-1)/2)
  G2 gen;
  Consts() {
    const F2 xi = F2{fq_small(9), fq_small(1)};
    b2 = f2_mul(F2{fq_small(3), fq_zero()}, f2_inv(xi));
    gamma2 = f2_pow(xi, Q_MINUS_1_OVER_3, 4);
    gamma3 = f2_pow(xi, Q_MINUS_1_OVER_2, 4);
    // the EIP-197 generator of G2
    const uint64_t gx0[4] = {0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull};
    const uint64_t gx1[4] = {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull};
    const uint64_t gy0[4] = {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull};
    const uint64_t gy1[4] = {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull};
    gen = G2{F2{fq_canon(gx0), fq_canon(gx1)}, F2{fq_canon(gy0), fq_canon(gy1)}, false};
  }
};
const Consts& consts() {
  static const Consts c;
  return c;
}

bool g2_on_curve(const G2& p) {
  if (p.inf) return true;
  return f2_eq(f2_mul(p.y, p.y), f2_add(f2_mul(f2_mul(p.x, p.x), p.x), consts().b2));
}
// r = r + q (r + r when q is r); with line != nullptr also the line through them evaluated at P = (xp, yp) on E(Fq12)
void g2_step(G2& r, const G2& q, const F* xp, const F* yp, F12* line) {
  if (line) *line = f12_one();
  if (q.inf) return;
  if (r.inf) {
    r = q;
    return;
  }
  F2 lambda;
  if (f2_eq(r.x, q.x)) {
    if (!f2_eq(r.y, q.y) || f2_is_zero(r.y)) {      // vertical: x_P - x_1 w^2; the sum is the identity
      if (line) {
        F12 l;
        for (int i = 0; i < 12; i++) l.c[i] = fq_zero();
        l.c[0] = *xp;
        f12_put(l, f2_neg(r.x), 2);
        *line = l;
      }
      r.inf = true;
      return;
    }
    const F2 xx = f2_mul(r.x, r.x);
    lambda = f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(r.y, r.y)));
  } else {
    lambda = f2_mul(f2_sub(q.y, r.y), f2_inv(f2_sub(q.x, r.x)));
  }
  if (line) {   // -y_P + (lambda x_P) w + (y_1 - lambda x_1) w^3
    F12 l;
    for (int i = 0; i < 12; i++) l.c[i] = fq_zero();
    l.c[0] = fq_neg(*yp);
    f12_put(l, f2_scale(lambda, *xp), 1);
    f12_put(l, f2_sub(r.y, f2_mul(lambda, r.x)), 3);
    *line = l;
  }
  const F2 x3 = f2_sub(f2_sub(f2_mul(lambda, lambda), r.x), q.x);
  const F2 y3 = f2_sub(f2_mul(lambda, f2_sub(r.x, x3)), r.y);
  r.x = x3;
  r.y = y3;
}
G2 g2_frobenius(const G2& p) {
  if (p.inf) return p;
  return G2{f2_mul(f2_conj(p.x), consts().gamma2), f2_mul(f2_conj(p.y), consts().gamma3), false};
}

// 6 x + 2 = 2^64 + ATE_LOW
const uint64_t ATE_LOW = 0x9d797039be763ba8ull;

F12 miller_loop(const G2& q, const F& xp, const F& yp) {
  F12 f = f12_one(), l;
  G2 r = q;
  for (int i = 63; i >= 0; i--) {
    f = f12_mul(f, f);
    g2_step(r, r, &xp, &yp, &l);
    f = f12_mul(f, l);
    if ((ATE_LOW >> i) & 1) {
      g2_step(r, q, &xp, &yp, &l);
      f = f12_mul(f, l);
    }
  }
  const G2 q1 = g2_frobenius(q);
  G2 nq2 = g2_frobenius(q1);
  nq2.y = f2_neg(nq2.y);
  g2_step(r, q1, &xp, &yp, &l);
  f = f12_mul(f, l);
  g2_step(r, nq2, &xp, &yp, &l);
  return f12_mul(f, l);
}

F12 final_exponentiation(const F12& f) {
  F12 acc = f12_one();
  for (int i = 64 * 44 - 1; i >= 0; i--) {
    acc = f12_mul(acc, acc);
    if ((FINAL_EXP[i / 64] >> (i % 64)) & 1) acc = f12_mul(acc, f);
  }
  return acc;
}

bool canonical_fq(const vdb_fq& v) { return lt_p(v.l, MQ.p); }
F as_f(const vdb_fq& v) { return F{{v.l[0], v.l[1], v.l[2], v.l[3]}}; }

}  // namespace

extern "C" {

int vdb_g2_mul_generator(const vdb_fr* s, vdb_g2* out) {
  if (!s || !out) {
    vdb::set_error("null pointer");
    return VDB_ERR_ARG;
  }
  // the canonical scalar: s / 2^256 mod r
  const F sc = mmul(F{{s->l[0], s->l[1], s->l[2], s->l[3]}}, F{{1, 0, 0, 0}}, MR);
  G2 acc = {F2{fq_zero(), fq_zero()}, F2{fq_zero(), fq_zero()}, true};
  for (int i = 255; i >= 0; i--) {
    g2_step(acc, acc, nullptr, nullptr, nullptr);
    if ((sc.v[i / 64] >> (i % 64)) & 1) g2_step(acc, consts().gen, nullptr, nullptr, nullptr);
  }
  memset(out, 0, sizeof(*out));
  if (!acc.inf) {
    memcpy(out->x[0].l, acc.x.a.v, 32);
    memcpy(out->x[1].l, acc.x.b.v, 32);
    memcpy(out->y[0].l, acc.y.a.v, 32);
    memcpy(out->y[1].l, acc.y.b.v, 32);
  }
  return VDB_OK;
}

int vdb_pairing_check(const vdb_g1* a, const vdb_g2* b, size_t n, int* ok) {
  if (!ok || (n && (!a || !b))) {
    vdb::set_error("null pointer");
    return VDB_ERR_ARG;
  }
  F12 f = f12_one();
  for (size_t i = 0; i < n; i++) {
    const vdb_g1& p = a[i];
    const vdb_g2& q = b[i];
    if (!canonical_fq(p.x) || !canonical_fq(p.y) || !canonical_fq(q.x[0]) || !canonical_fq(q.x[1]) || !canonical_fq(q.y[0]) ||
        !canonical_fq(q.y[1])) {
      vdb::set_error("vdb_pairing_check: pair %zu has a coordinate >= q", i);
      return VDB_ERR_ARG;
    }
    const F px = as_f(p.x), py = as_f(p.y);
    const bool p_inf = f_is_zero(px) && f_is_zero(py);
    const G2 qq = {F2{as_f(q.x[0]), as_f(q.x[1])}, F2{as_f(q.y[0]), as_f(q.y[1])}, false};
    const bool q_inf = f2_is_zero(qq.x) && f2_is_zero(qq.y);
    if (!p_inf && !f_eq(fq_mul(py, py), fq_add(fq_mul(fq_mul(px, px), px), fq_small(3)))) {
      vdb::set_error("vdb_pairing_check: G1 point %zu is not on the curve", i);
      return VDB_ERR_ARG;
    }
    if (!q_inf && !g2_on_curve(qq)) {
      vdb::set_error("vdb_pairing_check: G2 point %zu is not on the twist", i);
      return VDB_ERR_ARG;
    }
    if (p_inf || q_inf) continue;
    f = f12_mul(f, miller_loop(qq, px, py));
  }
  *ok = f12_is_one(final_exponentiation(f)) ? 1 : 0;
  return VDB_OK;
}

int vdb_g2_check(const vdb_g2* p, size_t n, int* ok) {
  if (!ok || (n && !p)) {
    vdb::set_error("null pointer");
    return VDB_ERR_ARG;
  }
  *ok = 1;
  for (size_t i = 0; i < n; i++) {
    const vdb_g2& q = p[i];
    if (!canonical_fq(q.x[0]) || !canonical_fq(q.x[1]) || !canonical_fq(q.y[0]) || !canonical_fq(q.y[1])) {
      *ok = 0;
      return VDB_OK;
    }
    const G2 pt = {F2{as_f(q.x[0]), as_f(q.x[1])}, F2{as_f(q.y[0]), as_f(q.y[1])}, false};
    if (f2_is_zero(pt.x) && f2_is_zero(pt.y)) continue;   // the identity
    if (!g2_on_curve(pt)) {
      *ok = 0;
      return VDB_OK;
    }
    // r P = O: the twist's group has order r times a large cofactor, so a point on it is in G2 only when this holds
    G2 acc = {F2{fq_zero(), fq_zero()}, F2{fq_zero(), fq_zero()}, true};
    for (int b = 253; b >= 0; b--) {
      g2_step(acc, acc, nullptr, nullptr, nullptr);
      if ((MR.p[b / 64] >> (b % 64)) & 1) g2_step(acc, pt, nullptr, nullptr, nullptr);
    }
    if (!acc.inf) {
      *ok = 0;
      return VDB_OK;
    }
  }
  return VDB_OK;
}

}  // extern "C"
