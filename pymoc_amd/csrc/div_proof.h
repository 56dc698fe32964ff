// div_proof.h -- the per-denominator proofs behind the kernels' 3- and 2-instruction exact
// quotients, and the operand pairs their device self tests run on.  Host arithmetic only: plain
// C++17, no HIP header, internal linkage throughout (used by exact_div.hip; any host compiler and
// its sanitizers can build it on its own).
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

namespace pm {
namespace {

// ---- the 3-instruction exact quotient by a static denominator, and its proof per denominator.
//   y = RN(1/d);   q0 = RN(a y);   r = RN(a - d q0) (one fma);   q = RN(q0 + r y) (one fma)
// With y = (1/d)(1 + e), |e| <= 2^-53, q0 lies within 1.5 ulp of x = a/d and the last fma rounds
// x + delta with |delta| <= |x - q0| (2 |e| + ...) < 3 * 2^-53 ulp (the residual may itself be
// rounded when q0 is more than an ulp off).  So q = RN(x) unless x lies within 3 * 2^-53 ulp of a
// rounding boundary, a midpoint (2K + 1) 2^(e-53) of two neighbours.  With 53-bit integer
// mantissas A, D of a, d:  x - midpoint = N / (2 D) ulp,  N = A 2^(53+t) - (2K + 1) D  (t = 0 for
// A >= D, 1 for A < D), an integer -- so only numerators with |N| <= 6 can fail, and for a GIVEN
// D these are the few solutions A of  A 2^(53+t) = N (mod D)  with an odd quotient (none at all
// when D has three or more trailing zero bits, as every difference of two grid levels has).
// div3_proof enumerates them and runs the very sequence on each, both signs: all equal to `/` =
// the quotient is correctly rounded for EVERY numerator (finite operands whose quotient and
// residual stay normal: the kernels' operand window, in_fast_div_range).  No denominator has
// failed in 10^8 tried (the cases that could are where q0 is a faithful quotient anyway), but the
// kernels take the 3-instruction form only on this proof, never on statistics.
inline double div3_host(double a, double d, double y) {
  const double q0 = a * y;
  const double r = __builtin_fma(-d, q0, a);
  return __builtin_fma(r, y, q0);
}
// The numerators that could fail for the denominator d: mantissas A with 0 < |N| <= nmax (nmax <= 7),
// handed to test(a, dm) as doubles a = A next to dm = D (d's mantissa as a double: the sequences are
// invariant under powers of two inside the operand window).  1: every test passed (or there was
// nothing to test); 0: a test failed, or d is zero / subnormal / not finite.  cand: if given, receives
// the candidates, ncand their count.
template <class Test>
int div_candidates_pass(double d, int nmax, Test test, std::vector<double> *cand, long long *ncand) {
  const double ad = d < 0 ? -d : d;
  if (!(ad >= 2.2250738585072014e-308 && ad <= 1.7976931348623157e308)) return 0;
  int e;
  const double m = frexp(ad, &e);                      // ad = m 2^e, m in [0.5, 1)
  const uint64_t D = (uint64_t)ldexp(m, 53);           // 53-bit mantissa
  const double dm = ldexp(m, 53);                      // the denominator the tests run on
  const int v = __builtin_ctzll(D);
  if (v >= 3) return 1;                                // |N| <= 7 has no multiple of 2^v: no candidate
  const uint64_t Dp = D >> v;
  if (Dp == 1) return 1;                               // a power of two
  int ok = 1;
  for (int t = 0; t < 2; ++t) {
    const int sh = 53 + t;
    for (int N = -nmax; N <= nmax; ++N) {
      if (N == 0 || (N % (1 << v)) != 0) continue;
      const int64_t Np = N / (1 << v);
      uint64_t x = (uint64_t)(((Np % (int64_t)Dp) + (int64_t)Dp) % (int64_t)Dp);
      for (int k = 0; k < sh - v; ++k) x = (x & 1) ? (x + Dp) / 2 : x / 2;  // Np 2^-(sh-v) mod Dp
      const uint64_t lo = t == 0 ? D : (1ull << 52), hi = t == 0 ? (1ull << 53) : D;
      const uint64_t k0 = lo > x ? (lo - x + Dp - 1) / Dp : 0;
      for (uint64_t A = x + k0 * Dp; A < hi; A += Dp) {
        const __int128 nn = (__int128)((unsigned __int128)A << sh) - N;
        if (nn % (__int128)D != 0 || ((nn / (__int128)D) & 1) == 0) continue;
        const double a = (double)A;
        if (ncand) ++*ncand;
        if (cand) cand->push_back(a);
        if (!test(a, dm)) ok = 0;  // (keeps enumerating: cand / ncand are the whole set)
      }
    }
  }
  return ok;
}
inline int div3_proof(double d, std::vector<double> *cand, long long *ncand) {
  return div_candidates_pass(
      d, 6,
      [](double a, double dm) {
        const double y = 1.0 / dm;
        return div3_host(a, dm, y) == a / dm && div3_host(-a, dm, y) == -a / dm;
      },
      cand, ncand);
}

// ---- the 2-instruction exact quotient by a static denominator, and its proof per denominator.
//   yh = RN(1/d);  yl = RN(e / d) with e = 1 - d yh (exact in one fma, |e| <= u = 2^-53);
//   u1 = RN(a yl);  q = RN(a yh + u1) (one fma)
// (common.hip.h: recip_lo_div, div_by_recip2x).  With yl = (e/d)(1 + d1) and u1 = a yl (1 + d2),
// |d1|, |d2| <= u, and yh = (1 - e)/d, the last fma rounds
//   s = a yh + u1 = x (1 - e) + x e (1 + d1)(1 + d2) = x (1 + eta),  x = a/d,
//   eta = e (d1 + d2 + d1 d2),  |eta| <= u^2 (2 + u) < 2.01 * 2^-106.
// x has a mantissa below 2^53 ulp, so |s - x| < 2.01 * 2^-53 ulp, and q = RN(s) = RN(x) unless a
// rounding midpoint lies between x and s.  In div3_proof's terms x - midpoint = N / (2 D) ulp with
// D < 2^53, i.e. more than |N| 2^-54 ulp: only numerators with |N| <= 4 can fail (|N| 2^-54 <
// 2.01 * 2^-53), none at all when D has three or more trailing zero bits.  div2_proof enumerates
// them with div3_proof's enumeration and runs the very sequence on each, both signs.  Unlike the
// 3-instruction form this one DOES fail for some denominators (about 1 % of uniform mantissas:
// there is no correction step, so a quotient 1 / (2 D) ulp off a midpoint on the wrong side of s
// stays wrong); those keep the 3-instruction form.  The verdict holds for the yh and yl formed
// here: the host's IEEE quotients, which the device must reproduce bit for bit (pm_recip2_check).
inline double div2_host(double a, double yh, double yl) {
  const double u1 = a * yl;
  return __builtin_fma(a, yh, u1);
}
// the host's yl for yh = RN(1/d) (common.hip.h: recip_lo_div is the device's)
inline double recip_lo_div_host(double d, double yh) { return __builtin_fma(-d, yh, 1.0) / d; }
inline int div2_proof(double d, std::vector<double> *cand, long long *ncand) {
  return div_candidates_pass(
      d, 4,
      [](double a, double dm) {
        const double yh = 1.0 / dm;
        const double yl = recip_lo_div_host(dm, yh);
        return div2_host(a, yh, yl) == a / dm && div2_host(-a, yh, yl) == -a / dm;
      },
      cand, ncand);
}

// ---- the operand pairs of the device self tests (pm_selftest_div3 / pm_selftest_div2)
struct DivPairs {
  std::vector<double> a, d;         // numerators, denominators
  std::vector<char> proven;         // the pair's denominator passed the proof
  unsigned long long unproven = 0;  // denominators that did not
};
using DivProof = int (*)(double d, std::vector<double> *cand, long long *ncand);

// `ndenoms` random denominators -- mantissas uniform, or a few units in the last place off 1 or 2
// (where the first product is worst), or with one or two trailing zero bits -- each with the
// candidate numerators of `proof`, both signs, rescaled (a rejected denominator's too, flagged in
// `proven`), and two arbitrary numerators: for every denominator, or with arbitrary_if_proven_only
// for those the proof accepts (the others then draw nothing, so the two settings walk the
// generator differently: each self test keeps the pairs its seeds have always given).
inline DivPairs selftest_div_pairs(uint64_t seed, int ndenoms, DivProof proof,
                                   bool arbitrary_if_proven_only) {
  DivPairs p;
  std::vector<double> c;
  unsigned long long st = seed ? seed : 1;
  auto next = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
  for (int i = 0; i < ndenoms; ++i) {
    const unsigned long long r = next();
    uint64_t D = (1ull << 52) | (next() >> 12);
    const int kind = (int)(r & 7);
    if (kind == 0) D = (1ull << 52) + 1 + (next() & 1023);
    if (kind == 1) D = (1ull << 53) - 1 - (next() & 1023);
    if (kind == 2) D &= ~1ull;
    if (kind == 3) D &= ~3ull;
    const double d = ldexp((double)D, -52 + (int)((r >> 8) % 41) - 20);
    c.clear();
    long long nc = 0;
    const int ok = proof(d, &c, &nc);
    if (!ok) ++p.unproven;
    const double scale = ldexp(1.0, (int)((r >> 16) % 41) - 20);
    auto add = [&](double a) {
      p.a.push_back(a);
      p.d.push_back(d);
      p.proven.push_back((char)ok);
    };
    for (double a : c) {
      add(a * scale);
      add(-a * scale);
    }
    if (ok || !arbitrary_if_proven_only)
      for (int k = 0; k < 2; ++k) {
        // (two statements: mantissa drawn before exponent, whatever the compiler's argument order)
        const uint64_t A = (1ull << 52) | (next() >> 12);
        add(ldexp((double)A, -40 - (int)(next() % 30)));
      }
  }
  return p;
}

}  // namespace
}  // namespace pm
