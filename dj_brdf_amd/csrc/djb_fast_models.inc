// djb_fast_models.inc -- part of djb_device.hpp (namespace djbdev; included ahead of the microfacet code, which uses fexp): the DECIDED fast tier of the sgd and abc models' fp64 terms (round 6).
//
// sgd::eval (dj_brdf.h:3416-3500) rounds nine doubles to float per pair -- g1 of i and of o and the ndf, per colour channel -- each the
// end of a chain of glibc's double pow and exp (sgd__g1: 1 + lambda (1 - exp(c pow(t1, k))), clamped to [0, 1]; sgd__ndf:
// kap exp(-ax) / pi / (pow(ax, p) c2 c2)): 9 pow + 9 exp as restated in djb_glibc_restated_f64.inc, ~1130 of the exact kernel's 1626
// VALU instructions per pair.  A float result does not need those doubles to the last place.  Here each chain is evaluated ONCE in
// plain double -- one table-driven logarithm (glibc's pow reduction and polynomial without its double-double tail) and one or two
// exponentials (glibc's exp reduction and polynomial, no special cases) -- together with a BOUND on the distance between this value
// and the reference's own double, accumulated per unit from the conditioning of every step (derivation at each function).  With
// y the fast value and B the bound, the reference's double lies in [y - B, y + B]; rounding to float (and the clamp) is monotone, so
// if both ends give the same float that float IS the reference's.  Otherwise -- and for anything outside the stated domains, NaNs
// included (every test is written so that a NaN fails it) -- the caller runs the exact chain.  Nothing is approximated in the result.
//
// Evidence: tools/sgd_fast_check.cpp (this file compiled for the host against the host's glibc and against __float128 values: the
// measured distance never exceeds 0.36 of the bound over the 100 published rows and 200 random rows; a CPU test runs it) and
// djb_selftest_model_fast (the device code against the exact device chain: decided / undecided / different -- the last must be 0;
// tools/model_fast_exhaustive.py: every float polar cosine of (0, 1] for every published row).
//
// The fast tier needs per-channel constants that depend on the row alone (logarithms of c and kap / pi, reciprocal of alpha, the
// bound's coefficients): sgd_fast_row() computes them on the host, create_model uploads them behind the 33 doubles of the row
// (SGD_FAST_* offsets); row[33] says whether the row is inside the fast tier's domain at all.

// fma with a literal addend in an SGPR pair on the device (fma_sk, djb_device.hpp), a plain fma on the host (check tool)
#if defined(DJB_HOST_MATH)
#define DJB_FMK(a, b, k) __builtin_fma((a), (b), (k))
#else
#define DJB_FMK(a, b, k) fma_sk((a), (b), (k))
#endif

enum { SGD_FAST_FLAG = 33, SGD_FAST_LNC = 34, SGD_FAST_E0 = 37, SGD_FAST_RHO_L = 40, SGD_FAST_RHO_K = 43,
       SGD_FAST_LNKPI = 46, SGD_FAST_INV_ALPHA = 49, SGD_FAST_B_L = 52, SGD_FAST_B_K = 55, SGD_FAST_RHO_T = 58, SGD_FAST_ROW = 61 };
constexpr double SGD_U = 0x1p-53;               // half an ulp of a double in [1, 2): one rounding

// ln(x) for a positive NORMAL double: the reduction, table and polynomial of glibc's pow (log_inline, e_pow.c) in plain double.
// x = 2^k z, z in [0x1.69555p-1, 0x1.69555p0), c = the table centre of z's sub-interval: ln x = k ln2 + ln c + log1p(r), r = z / c - 1
// (|r| < 0x1.3p-7), log1p(r) = r + r^2 P(r).  Error: one rounding each of t1 = k Ln2hi + logc, of t1 + r and of the final sum -- the
// low parts (k Ln2lo + logctail, r^2 P) enter below 2^-60 -- so |flog(x) - ln x| <= 3 * 2^-53 |ln x| + 2^-59; the callers use
// 2^-51 |L| + 2^-57 (tools/sgd_fast_check.cpp measures 2.0 * (2^-53 |L| + 2^-62) at worst over 4e8 arguments).
DJB_DEV double flog(double x, LdsTab PT)
{
	constexpr double Ln2hi = DJB_GLIBC_POW_C[0], Ln2lo = DJB_GLIBC_POW_C[1];
	// glibc's A[i] are scaled for its own evaluation order (ar = -r/2 ...): as plain coefficients of r^3 .. r^8 (exact rescalings)
	constexpr double C3 = -0.5 * DJB_GLIBC_POW_C[3], C4 = -0.5 * DJB_GLIBC_POW_C[4], C5 = 0.25 * DJB_GLIBC_POW_C[5],
	                 C6 = 0.25 * DJB_GLIBC_POW_C[6], C7 = -0.125 * DJB_GLIBC_POW_C[7], C8 = -0.125 * DJB_GLIBC_POW_C[8];
	const unsigned int hx = (unsigned int)__double2hiint(x);
	const unsigned int tmph = hx - 0x3fe69555u;
	const int i = (int)((tmph >> 13) & 127u);
	const int k = (int)tmph >> 20;
	const double z = __hiloint2double((int)(hx - (tmph & 0xfff00000u)), __double2loint(x));
	const double kd = (double)k;
	double invc, logc, logctail;
	if (PT) { lds_f64p L = (lds_f64p)(uintptr_t)(PT - 1u) + 3 * i; invc = L[0]; logc = L[1]; logctail = L[2]; }
	else { const double *T = DJB_GLIBC_POW_LOG_TAB + 3 * i; invc = T[0]; logc = T[1]; logctail = T[2]; }
	const double r = __builtin_fma(z, invc, -1.0);
	const double t1 = __builtin_fma(kd, Ln2hi, logc);
	const double lo1 = __builtin_fma(kd, Ln2lo, logctail);
	double p = DJB_FMK(r, C8, C7);
	p = DJB_FMK(r, p, C6);
	p = DJB_FMK(r, p, C5);
	p = DJB_FMK(r, p, C4);
	p = DJB_FMK(r, p, C3);
	p = DJB_FMK(r, p, -0.5);
	return (t1 + r) + __builtin_fma(r * r, p, lo1);
}
// e^x for |x| <= 708: glibc's exp (e_exp.c) main path -- k = round(x N / ln2), r = x - k ln2 / N, 2^(k/N) from the 128-entry table,
// degree-5 polynomial -- without its special cases.  Relative error <= 2^-52 (glibc states 0.511 ulp for the same operations; the
// callers use 2^-51).
DJB_DEV double fexp(double x, LdsTab T)
{
	unsigned int klo, sh; int sl;
	const double tmp = glibc_exp_tmp(x, 0.0, klo, sh, sl, T);
	const double scale = __hiloint2double((int)sh, sl);
	return __builtin_fma(scale, tmp, scale);
}
#if defined(DJB_HOST_MATH)
DJB_DEV double recip_fast_m(double q) { const double r = D(1.0f / F(q)); const double e = __builtin_fma(-q, r, 1.0); return __builtin_fma(r, __builtin_fma(e, e, e), r); }
DJB_DEV float med01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }       // not reached with a NaN that matters: NaN != NaN below
#else
DJB_DEV double recip_fast_m(double q) { return recip_fast(q); }
DJB_DEV float med01(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }
#endif

// ---- sgd__g1 (dj_brdf.h:3416-3422): float(min(1, max(0, 1 + lambda (1 - exp(c pow(t1, k)))))), t1 = max(0, theta_k - theta0) as the
// caller's d = theta_k - theta0 gives it.  Domain (sgd_fast_row): c, lambda > 0, 1 <= k <= 4096, |theta0| <= 4.
//   t1 == 0: pow(+0, k) = +0, exp(0) = 1, every later step exact: 1.0f.
//   else  L = flog(t1), a = k L + ln c, E = e^a against the reference's E_r = RN(c pow(t1, k)):  |E - E_r| <= E rho,
//           rho = k dL + U (|a| + |ln c| + 1) [the fma, the host's ln c] + 2^-51 [fexp] + 3U [glibc's pow, the product],
//           dL = 2^-51 |L| + 2^-57  =>  rho <= U (5 k |L| + 2 |ln c| + k / 16 + 8) =: rho_l |L| + rho_k  (both per channel; < 2^-33)
//         E >= E0 = (1 + 2^-30) ln(1 + 3 / lambda): lambda (e^E_r - 1) >= 2, the reference's sum is <= -1 (or -inf): +0.
//         else Y = e^E, t2 = 1 - Y, t3 = fma(lambda, t2, 1) against the reference's RN(1 + RN(lambda RN(1 - exp(E_r)))):
//           |Y - Y_r| <= Y (1.01 E rho + 3U) (fexp and glibc's exp: ~1.1U each),  the subtractions add U |t2| each, the reference's
//           product U lambda |t2|, the sums U |t3| each, |t3| <= 1 + lambda |t2|:
//               B <= lambda (Y (1.01 E rho + 3U) + 5U |t2|) + 2U
//         the bound used is TWICE that: lambda (Y (2.1 E rho + 6U) + 10U |t2|) + 4U; the factor 2.1 is folded into rho_l, rho_k.
//         (|t2| is kept, not bounded by Y + 1: lambda reaches 1.5e7 in the published rows, and a pair far from the wall has t2 = 0.)
// TH_APPROX (the kernels' theta_k from the arctangent core, djb_device.hpp: acos_fast, within 5 ulp64 of glibc's acos as measured by
// djb_selftest_fast_trig): d = theta_k - theta0 then differs from the reference's difference by at most unc = dth + 2^-49 (dth: the caller's
// bound on theta_k, 1.01 * 2^-48 theta_k -- three times the measured distance; 2^-49: the two roundings of the subtraction for |theta|,
// |theta0| <= 4).  d <= -unc: the reference's t1 is 0.  d > 0: t1 = d carries a relative error unc / d, k times that in a: rho grows by
// rho_t unc / d (rho_t = 2.1 * 1.05 k; the reciprocal from v_rcp_f32, 1e-7), and a unit whose rho exceeds 2^-20 -- d within 2^-28 of the
// wall -- is undecided (the linearisations above want E rho << 1).  With the reference's own theta_k (TH_APPROX = false) unc = 0.
// Returns the float, decided = true; or decided = false (the value is then meaningless).
template <bool TH_APPROX>
DJB_DEV float sgd_g1_fast(const double *m, int ch, double d, double dth, LdsTab PT, LdsTab ET, bool &decided, double *dbg = nullptr)
{
	const double unc = TH_APPROX ? dth + 0x1p-49 : 0.0;
	const bool one = d <= -unc;                                     // theta_k <= theta0: t1 = +0 in the reference
	const double L = flog(d, PT);
	const double aL = L < 0.0 ? -L : L;
	const double a = __builtin_fma(m[27 + ch], L, m[SGD_FAST_LNC + ch]);
	const double E = fexp(dmin_(dmax_(a, -700.0), 6.6), ET);        // a > 6.6: E > 735 > any E0 (lambda >= 1e-200)
	double rho = __builtin_fma(m[SGD_FAST_RHO_L + ch], aL, m[SGD_FAST_RHO_K + ch]);
	if (TH_APPROX) {
#if defined(DJB_HOST_MATH)
		const double rd = D(1.0f / F(d));
#else
		const double rd = D(__builtin_amdgcn_rcpf(F(d)));
#endif
		rho = __builtin_fma(m[SGD_FAST_RHO_T + ch] * unc, rd, rho);
	}
	const double E0 = m[SGD_FAST_E0 + ch], lam = m[21 + ch];
	const bool zero = E >= E0;
	const double Y = fexp(dmin_(E, E0), ET);
	const double t2 = 1.0 - Y, at2 = t2 < 0.0 ? -t2 : t2;
	const double t3 = __builtin_fma(lam, t2, 1.0);
	const double B = __builtin_fma(lam, __builtin_fma(10.0 * SGD_U, at2, Y * __builtin_fma(E, rho, 6.0 * SGD_U)), 4.0 * SGD_U);
	if (dbg) { dbg[0] = t3; dbg[1] = B; dbg[2] = zero ? 1.0 : 0.0; }
	const float lo = med01(F(t3 - B)), hi = med01(F(t3 + B));
	decided = one | ((zero | (lo == hi)) & (d > 0x1p-1000) & (a == a) & (rho < 0x1p-20));
	return one ? 1.0f : (zero ? 0.0f : lo);
}
// ---- sgd__ndf (dj_brdf.h:3424-3432): float(kap exp(-ax) inv_pi / (pow(ax, p) c2 c2)), c2 = ch^2, ax = alpha + ((1 - c2) / c2) / alpha.
// Domain (sgd_fast_row): alpha, kap > 0, 0 <= p <= 1024; per unit 2^-30 <= c2 <= 2, 2^-100 <= ax <= 2^100 (else undecided).
//   c2 and 1 - c2 are the reference's; the caller passes t2 = (1 - c2) rc and rc2 = rc rc, rc = recip_fast(c2) (3U): ax = fma(t2, RN(1 / alpha), alpha): |ax - ax_r| <= 10U ax.
//   With T(ax) = (kap / pi) e^-ax ax^-p / c2^2:  |ln T(ax) - ln T(ax_r)| <= (ax + p) 10U;  the reference's evaluation of T(ax_r) (exp, pow,
//   three products, inv_pi, the division) is within 10U of it;  the fast one is exp(X) rc rc, X = fma(-p, L, ln(kap / pi) - ax),
//   L = flog(ax): |X - ln(..)| <= p dL + U (|s| + |X| + |ln(kap/pi)| + 2), then fexp 2^-51 and the two products by rc 8U.
//   Sum <= U (12 ax + 11 p + 3 p |L| + 3 |ln(kap/pi)| + 22); the bound used is TWICE that, as a relative bound b on the value:
//       b = 2^-52 (12 ax + 4 p |L| + 16 p + 4 |ln(kap/pi)| + 32) =: 12 * 2^-52 ax + b_l |L| + b_k.
//   X < -700 is clamped: the value is then below 1e-280 either way and both ends round to +0.
DJB_DEV float sgd_ndf_fast(const double *m, int ch, double c2, double t2, double rc2, LdsTab PT, LdsTab ET, bool &decided, double *dbg = nullptr)
{
	const double ax = __builtin_fma(t2, m[SGD_FAST_INV_ALPHA + ch], m[6 + ch]);
	const double L = flog(ax, PT);
	const double aL = L < 0.0 ? -L : L;
	const double X = __builtin_fma(-m[9 + ch], L, m[SGD_FAST_LNKPI + ch] - ax);
	const double V = fexp(dmin_(dmax_(X, -700.0), 700.0), ET) * rc2;
	const double b = __builtin_fma(12.0 * 0x1p-52, ax, __builtin_fma(m[SGD_FAST_B_L + ch], aL, m[SGD_FAST_B_K + ch]));
	// the reference's value is a quotient of positive terms: never below +0.  Without the clamp a bound b > 1 (ax above 3.7e14, where
	// e^-ax is long +0: a user's row with alpha = 1e-12) put the lower end below zero, F() made it -0, and -0 == +0 decided it
	const float lo = F(dmax_(__builtin_fma(V, -b, V), 0.0)), hi = F(__builtin_fma(V, b, V));
	if (dbg) { dbg[0] = V; dbg[1] = b; }
	decided = (lo == hi) & (hi < 3e38f) & (ax >= 0x1p-100) & (ax <= 0x1p100) & (c2 >= 0x1p-30) & (c2 <= 2.0) & (X < 700.0);
	return lo;
}
// ---- abc__ndf (dj_brdf.h:3608-3613): float(A / pow(w, C)), w = 1 + B (1 - cos_theta_h) (the reference's own double), three A per unit.
// q = e^(-C L), L = flog(w):  |ln q + C ln w| <= C dL + U |C L| + 2^-51 [fexp];  the product A q adds U;  the reference's pow and division
// 3U:  sum <= U (5 C |L| + C / 16 + 10);  the bound used is TWICE that, relative: b = 2^-52 (5 C |L| + C / 16 + 10).
// Domain: 0 <= C <= 4096 (launch-uniform), 2^-100 <= w <= 2^100, |C L| < 700; anything else (NaNs included) is undecided.
DJB_DEV void abc_ndf_fast(const double *m, double w, LdsTab PT, LdsTab ET, float (&v)[3], bool (&decided)[3], double *dbg = nullptr)
{
	const double C = m[7];
	const double L = flog(w, PT);
	const double aL = L < 0.0 ? -L : L;
	const double X = -C * L;
	const double q = fexp(dmin_(dmax_(X, -700.0), 700.0), ET);
	const double b = __builtin_fma(0x1p-52 * 5.0 * C, aL, 0x1p-52 * (C * 0.0625 + 10.0));
	const bool in = (C >= 0.0) & (C <= 4096.0) & (w >= 0x1p-100) & (w <= 0x1p100) & (X > -700.0) & (X < 700.0);
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const double V = m[3 + c] * q;
		const float lo = F(__builtin_fma(V, -b, V)), hi = F(__builtin_fma(V, b, V));
		v[c] = lo;
		decided[c] = in & (lo == hi) & (fabsf(hi) < 3e38f);
		if (dbg) { dbg[2 * c] = V; dbg[2 * c + 1] = b; }
	}
}
// the constants behind the row (host; doubles 33 .. SGD_FAST_ROW - 1 of the device copy).  Returns false -- and clears the flag -- when a
// channel is outside the fast tier's domain: the kernels then run the exact chains only.
static inline bool sgd_fast_row(const double *row, double *out /* [SGD_FAST_ROW] */)
{
	bool ok = true;
	for (int j = 0; j < 33; ++j) out[j] = row[j];
	for (int j = 33; j < SGD_FAST_ROW; ++j) out[j] = 0.0;
	for (int ch = 0; ch < 3; ++ch) {
		const double alpha = row[6 + ch], p = row[9 + ch], kap = row[18 + ch], lam = row[21 + ch], c = row[24 + ch], k = row[27 + ch], th0 = row[30 + ch];
		ok = ok && alpha >= 1e-12 && alpha <= 1e12 && p >= 0.0 && p <= 1024.0 && kap >= 1e-100 && kap <= 1e100 && lam >= 1e-200 && lam <= 1e100
		        && c >= 1e-300 && c <= 1e300 && k >= 1.0 && k <= 4096.0 && th0 >= -4.0 && th0 <= 4.0;
		if (!ok) break;
		const double lnc = log(c), lnkpi = log(kap / DJB_PI);
		out[SGD_FAST_LNC + ch] = lnc;
		out[SGD_FAST_E0 + ch] = (1.0 + 0x1p-30) * log1p(3.0 / lam);
		out[SGD_FAST_RHO_L + ch] = 2.1 * SGD_U * 5.0 * k;
		out[SGD_FAST_RHO_K + ch] = 2.1 * SGD_U * (2.0 * fabs(lnc) + k / 16.0 + 8.0);
		out[SGD_FAST_RHO_T + ch] = 2.1 * 1.05 * k;
		out[SGD_FAST_LNKPI + ch] = lnkpi;
		out[SGD_FAST_INV_ALPHA + ch] = 1.0 / alpha;
		out[SGD_FAST_B_L + ch] = 0x1p-52 * 4.0 * p;
		out[SGD_FAST_B_K + ch] = 0x1p-52 * (16.0 * p + 4.0 * fabs(lnkpi) + 32.0);
	}
	out[SGD_FAST_FLAG] = ok ? 1.0 : 0.0;
	return ok;
}
