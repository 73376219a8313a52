// utia_set_facade.cpp -- djb::utia_set of the djb:: facade (include/djb_hip.hpp): two UTIA tables built in memory, a set of them, and
// eval / evalp of a batch of hits (inactive ones included) held, bit for bit, against the two djb::utia objects' own eval / evalp.
// tests/test_utia_set_host.py runs it on the CPU context (DJB_DEVICE=cpu).  Prints "<n> hits checked, <d> differ"; exit 1 if d != 0.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "dj_brdf.h"

static unsigned int bits(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }

int main()
{
	const size_t N = 3 * 288 * 288;
	std::vector<double> ta(N), tb(N);
	unsigned int h = 12345u;
	for (size_t k = 0; k < N; ++k) {
		h = h * 1664525u + 1013904223u;
		ta[k] = 20.0 + 90.0 * (double)(k % 48) / 48.0 + (double)(k % 7);
		tb[k] = 125.0 * (double)(h >> 8) / 16777216.0 - 2.0;
	}
	const int n = 600;
	std::vector<djb::vec3> i(n), o(n), got(n), one(n);
	std::vector<int32_t> ids(n);
	for (int k = 0; k < n; ++k) {
		// directions over the upper hemisphere, on and off the table's grid lines
		const float ti = 1.5f * (float)((k * 7) % 58), pi_ = 7.5f * (float)((k * 5) % 48) + (k % 3 ? 0.37f * (float)(k % 11) : 0.0f);
		const float to = 1.5f * (float)((k * 11) % 58), po = 7.5f * (float)((k * 13) % 48) + (k % 4 ? 0.53f * (float)(k % 7) : 0.0f);
		const float r = 0.017453292f;
		i[k] = djb::vec3(std::sin(ti * r) * std::cos(pi_ * r), std::sin(ti * r) * std::sin(pi_ * r), std::cos(ti * r));
		o[k] = djb::vec3(std::sin(to * r) * std::cos(po * r), std::sin(to * r) * std::sin(po * r), std::cos(to * r));
		const int32_t cycle[5] = { 0, 1, -1, 1, 2 };          // 2 and -1: inactive
		ids[k] = cycle[k % 5];
	}
	djb::utia a(ta.data()), b(tb.data());
	djb::utia_set *set;
	{
		djb::utia a2(ta.data()), b2(tb.data());
		const djb::utia *members[2] = { &a2, &b2 };
		set = new djb::utia_set(2, members);               // the members go out of scope: the set holds copies of their tables
	}
	if (set->size() != 2) return 3;
	int differ = 0, checked = 0, nonzero = 0;
	for (int cosine = 0; cosine < 2; ++cosine) {
		if (cosine) set->evalp((size_t)n, ids.data(), &i[0], &o[0], &got[0]);
		else set->eval((size_t)n, ids.data(), &i[0], &o[0], &got[0]);
		for (int k = 0; k < n; ++k) {
			djb::vec3 want(0, 0, 0);
			if (ids[k] == 0 || ids[k] == 1) {
				const djb::brdf &m = ids[k] ? (const djb::brdf &)b : (const djb::brdf &)a;
				want = cosine ? m.evalp(i[k], o[k]) : m.eval(i[k], o[k]);
			}
			++checked;
			if (bits(got[k].x) != bits(want.x) || bits(got[k].y) != bits(want.y) || bits(got[k].z) != bits(want.z)) ++differ;
			if (want.x != 0.0f) ++nonzero;
		}
	}
	delete set;
	printf("%d hits checked, %d differ, %d non-zero\n", checked, differ, nonzero);
	return differ == 0 && nonzero > checked / 4 ? 0 : 1;
}
