// scene_facade.cpp -- djb::scene of the djb:: facade (include/djb_hip.hpp): a scene over an sgd model set built from two djb::sgd objects
// and an abc model set built from two explicit rows, slots {sgd 0, abc 1, none, sgd 1, abc 0, sgd 0}; eval / evalp of a batch of hits
// (ids outside the table and on the slot without material included) held, bit for bit, against the single-material objects' own
// eval / evalp (djb::sgd, and djb_brdf_create_abc_from_params objects through the C ABI).
// tests/test_scene_host.py runs it on the CPU context (DJB_DEVICE=cpu).  Prints "<n> hits checked, <d> differ"; exit 1 if d != 0.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include "dj_brdf.h"

static unsigned int bits(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }
static bool same(const djb::vec3 &a, const djb::vec3 &b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y) && bits(a.z) == bits(b.z); }

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
		const int32_t cycle[9] = { 0, 1, 2, 3, 4, 5, -1, 6, 3 };          // 2: the slot without material; -1 and 6: outside the table
		ids[k] = cycle[k % 9];
	}
	djb::sgd a("gold-metallic-paint"), b("blue-acrylic");
	const djb::sgd *members[2] = { &a, &b };
	djb::model_set sgd_set(2, members);
	const double rows[2][9] = { { 0.02, 0.05, 0.11, 30.0, 24.0, 18.5, 900.0, 0.9, 1.4 }, { 0.3, 0.1, 0.05, 1.5, 2.5, 3.5, 40.0, 1.7, 2.1 } };      // kD[3] A[3] B C ior
	djb::model_set abc_set(DJB_KIND_ABC, 2, &rows[0][0]);
	const djb_scene_slot slots[6] = { { DJB_KIND_SGD, 0 }, { DJB_KIND_ABC, 1 }, { DJB_SCENE_NONE, 0 }, { DJB_KIND_SGD, 1 }, { DJB_KIND_ABC, 0 }, { DJB_KIND_SGD, 0 } };
	djb::scene *first = new djb::scene(NULL, NULL, &sgd_set, &abc_set, 6, slots);
	djb::scene sc(std::move(*first));                           // move-only
	delete first;
	if (sc.size() != 6 || sc.members(0) != 0 || sc.members(1) != 0 || sc.members(2) != 2 || sc.members(3) != 2) return 3;
	try {                                                       // a slot that names an absent set is refused with the slot's number
		const djb_scene_slot bad[2] = { { DJB_KIND_SGD, 0 }, { DJB_KIND_MERL, 0 } };
		djb::scene refused(NULL, NULL, &sgd_set, NULL, 2, bad);
		return 4;
	} catch (const djb::exc &e) {
		if (!strstr(e.what(), "slot 1")) return 5;
	}
	djb_ctx *ctx = djb::hip::context::standard().get();
	djb_brdf *abc_single[2] = { NULL, NULL };
	for (int m = 0; m < 2; ++m) if (djb_brdf_create_abc_from_params(ctx, rows[m], &abc_single[m]) != DJB_OK) return 6;
	int differ = 0, checked = 0, nonzero = 0;
	std::vector<djb::vec3> abc_want[2] = { std::vector<djb::vec3>(n), std::vector<djb::vec3>(n) };
	for (int cosine = 0; cosine < 2; ++cosine) {
		if (cosine) sc.evalp((size_t)n, ids.data(), &i[0], &o[0], &got[0]);
		else sc.eval((size_t)n, ids.data(), &i[0], &o[0], &got[0]);
		for (int m = 0; m < 2; ++m) {
			djb_vec3_view vi = djb::hip::view(&i[0]), vo = djb::hip::view(&o[0]), vw = djb::hip::view(&abc_want[m][0]);
			if ((cosine ? djb_evalp_batch : djb_eval_batch)(ctx, abc_single[m], n, &vi, &vo, NULL, &vw, DJB_MEM_HOST) != DJB_OK) return 7;
		}
		for (int k = 0; k < n; ++k) {
			djb::vec3 want(0, 0, 0);
			const int32_t id = ids[k];
			if (id >= 0 && id < 6 && slots[id].kind == DJB_KIND_SGD) {
				const djb::brdf &m = slots[id].local ? (const djb::brdf &)b : (const djb::brdf &)a;
				want = cosine ? m.evalp(i[k], o[k]) : m.eval(i[k], o[k]);
			} else if (id >= 0 && id < 6 && slots[id].kind == DJB_KIND_ABC) want = abc_want[slots[id].local][k];
			++checked;
			if (!same(got[k], want)) ++differ;
			if (want.x != 0.0f) ++nonzero;
		}
	}
	for (int m = 0; m < 2; ++m) djb_brdf_destroy(abc_single[m]);
	printf("%d hits checked, %d differ, %d non-zero\n", checked, differ, nonzero);
	return differ == 0 && nonzero > checked / 4 ? 0 : 1;
}
