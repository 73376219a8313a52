// proxy_is_facade.cpp -- brdf::evalp_is_proxy of the djb:: facade (include/djb_hip.hpp), scalar and batch members, for two pairs; prints
// weight, direction and pdf of every unit as hex floats.  tests/test_proxy_is_host.py runs it on the CPU context (DJB_DEVICE=cpu) and
// holds the lines against the Python mirror's results for the same inputs.
#include <cstdio>
#include <vector>
#include "dj_brdf.h"

static void show(const char *tag, const djb::vec3 &w, const djb::vec3 &i, float pdf)
{
	printf("%s %a %a %a %a %a %a %a\n", tag, w.x, w.y, w.z, i.x, i.y, i.z, pdf);
}

int main()
{
	const int n = 5;
	const float u1[n] = { 0.1f, 0.35f, 0.5f, 0.75f, 0.9f }, u2[n] = { 0.8f, 0.6f, 0.45f, 0.2f, 0.05f };
	const float dir[n][3] = { { 0.1f, 0.3f, 0.9486833f }, { 0.3f, 0.2f, 0.9327379f }, { 0.5f, 0.1f, 0.8602325f }, { 0.7f, 0.0f, 0.7141428f },
	                          { 0.9f, -0.1f, 0.4242641f } };
	std::vector<djb::vec3> o(n), w(n), i(n);
	std::vector<float> pdf(n);
	for (int k = 0; k < n; ++k) o[k] = djb::vec3(dir[k][0], dir[k][1], dir[k][2]);
	djb::abc abc("gold-metallic-paint");
	djb::sgd sgd("gold-metallic-paint");
	djb::ggx ggx;
	djb::beckmann beckmann;
	const djb::microfacet::params pg = djb::microfacet::params::elliptic(0.2f, 0.5f, 0.7f), pb = djb::microfacet::params::isotropic(0.3f);
	for (int k = 0; k < n; ++k) {
		djb::vec3 ik; float pk;
		const djb::vec3 wk = abc.evalp_is_proxy(ggx, u1[k], u2[k], o[k], &ik, &pk, NULL, &pg);
		show("abc_ggx_scalar", wk, ik, pk);
	}
	abc.evalp_is_proxy(ggx, (size_t)n, u1, u2, &o[0], &w[0], &i[0], &pdf[0], NULL, &pg);
	for (int k = 0; k < n; ++k) show("abc_ggx_batch", w[k], i[k], pdf[k]);
	for (int k = 0; k < n; ++k) {
		djb::vec3 ik; float pk;
		const djb::vec3 wk = sgd.evalp_is_proxy(beckmann, u1[k], u2[k], o[k], &ik, &pk, NULL, &pb);
		show("sgd_beckmann_scalar", wk, ik, pk);
	}
	sgd.evalp_is_proxy(beckmann, (size_t)n, u1, u2, &o[0], &w[0], &i[0], &pdf[0], NULL, &pb);
	for (int k = 0; k < n; ++k) show("sgd_beckmann_batch", w[k], i[k], pdf[k]);
	return 0;
}
