// model_set_facade.cpp -- djb::model_set of the djb:: facade (include/djb_hip.hpp): a set built from two djb::sgd objects and a set built
// from two explicit abc rows; eval / evalp of a batch of hits (inactive ones included) held, bit for bit, against the single-material
// objects' own eval / evalp (djb::sgd, and djb_brdf_create_abc_from_params objects through the C ABI).
// tests/test_model_set_host.py runs it on the CPU context (DJB_DEVICE=cpu).  Prints "<n> hits checked, <d> differ"; exit 1 if d != 0.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "dj_brdf.h"

static unsigned int bits(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }

int main()
{
	const int n = 600;
	std::vector<djb::vec3> i(n), o(n), got(n);
	std::vector<int32_t> ids(n);
	for (int k = 0; k < n; ++k) {
		const float ti = 1.5f * (float)((k * 7) % 64), pi_ = 7.5f * (float)((k * 5) % 48) + 0.37f * (float)(k % 11);      // up to 94.5 degrees: some below the horizon
		const float to = 1.5f * (float)((k * 11) % 64), po = 7.5f * (float)((k * 13) % 48) + 0.53f * (float)(k % 7);
		const float r = 0.017453292f;
		i[k] = djb::vec3(std::sin(ti * r) * std::cos(pi_ * r), std::sin(ti * r) * std::sin(pi_ * r), std::cos(ti * r));
		o[k] = djb::vec3(std::sin(to * r) * std::cos(po * r), std::sin(to * r) * std::sin(po * r), std::cos(to * r));
		const int32_t cycle[5] = { 0, 1, -1, 1, 2 };          // 2 and -1: inactive
		ids[k] = cycle[k % 5];
	}
	int differ = 0, checked = 0, nonzero = 0;
	// ---- from objects
	djb::sgd a("gold-metallic-paint"), b("blue-acrylic");
	djb::model_set *set;
	{
		djb::sgd a2("gold-metallic-paint"), b2("blue-acrylic");
		const djb::sgd *members[2] = { &a2, &b2 };
		set = new djb::model_set(2, members);               // the members go out of scope: the set holds copies of their rows
	}
	if (set->size() != 2 || set->kind() != DJB_KIND_SGD) return 3;
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
	djb::model_set moved(std::move(*set));                      // move-only
	delete set;
	if (moved.size() != 2) return 4;
	// ---- from rows: kD[3] A[3] B C ior
	const double rows[2][9] = { { 0.02, 0.05, 0.11, 30.0, 24.0, 18.5, 900.0, 0.9, 1.4 }, { 0.3, 0.1, 0.05, 1.5, 2.5, 3.5, 40.0, 1.7, 2.1 } };
	djb::model_set abc_set(DJB_KIND_ABC, 2, &rows[0][0]);
	if (abc_set.size() != 2 || abc_set.kind() != DJB_KIND_ABC) return 5;
	djb_ctx *ctx = djb::hip::context::standard().get();
	djb_brdf *single[2] = { NULL, NULL };
	for (int m = 0; m < 2; ++m) if (djb_brdf_create_abc_from_params(ctx, rows[m], &single[m]) != DJB_OK) return 6;
	std::vector<djb::vec3> want(n);
	abc_set.evalp((size_t)n, ids.data(), &i[0], &o[0], &got[0]);
	for (int m = 0; m < 2; ++m) {
		djb_vec3_view vi = djb::hip::view(&i[0]), vo = djb::hip::view(&o[0]), vw = djb::hip::view(&want[0]);
		if (djb_evalp_batch(ctx, single[m], n, &vi, &vo, NULL, &vw, DJB_MEM_HOST) != DJB_OK) return 7;
		for (int k = 0; k < n; ++k) {
			if (ids[k] != m) continue;
			++checked;
			if (bits(got[k].x) != bits(want[k].x) || bits(got[k].y) != bits(want[k].y) || bits(got[k].z) != bits(want[k].z)) ++differ;
			if (want[k].x != 0.0f) ++nonzero;
		}
		djb_brdf_destroy(single[m]);
	}
	for (int k = 0; k < n; ++k)
		if (ids[k] != 0 && ids[k] != 1) { ++checked; if (bits(got[k].x) | bits(got[k].y) | bits(got[k].z)) ++differ; }
	printf("%d hits checked, %d differ, %d non-zero\n", checked, differ, nonzero);
	return differ == 0 && nonzero > checked / 4 ? 0 : 1;
}
