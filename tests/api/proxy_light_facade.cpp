// proxy_light_facade.cpp -- brdf::evalp_pdf_proxy of the djb:: facade (include/djb_hip.hpp), scalar and batch members, for two pairs of
// objects on five fixed pairs of directions (one with i.z < 0, one with o.z < 0, three live); prints fr and pdf of every unit as hex
// floats.  tests/test_proxy_light_host.py runs it on the CPU context (DJB_DEVICE=cpu) and holds the lines against the Python mirror's
// results for the same inputs.
#include <cstdio>
#include <vector>
#include "dj_brdf.h"

static void show(const char *tag, const djb::vec3 &fr, float pdf)
{
	printf("%s %a %a %a %a\n", tag, fr.x, fr.y, fr.z, pdf);
}

int main()
{
	const int n = 5;
	const float od[n][3] = { { 0.1f, 0.3f, 0.9486833f }, { 0.3f, 0.2f, 0.9327379f }, { 0.5f, 0.1f, 0.8602325f }, { 0.7f, 0.0f, 0.7141428f },
	                         { 0.9f, -0.1f, -0.4242641f } };
	const float id[n][3] = { { -0.1f, -0.25f, 0.9630680f }, { -0.3f, -0.2f, -0.9327379f }, { 0.1f, 0.5f, 0.8602325f }, { -0.6f, 0.1f, 0.7937254f },
	                         { 0.2f, 0.2f, 0.9591663f } };
	std::vector<djb::vec3> i(n), o(n), fr(n);
	std::vector<float> pdf(n);
	for (int k = 0; k < n; ++k) { i[k] = djb::vec3(id[k][0], id[k][1], id[k][2]); o[k] = djb::vec3(od[k][0], od[k][1], od[k][2]); }
	djb::abc abc("gold-metallic-paint");
	djb::sgd sgd("gold-metallic-paint");
	djb::ggx ggx;
	djb::beckmann beckmann;
	const djb::microfacet::params pg = djb::microfacet::params::elliptic(0.2f, 0.5f, 0.7f), pb = djb::microfacet::params::isotropic(0.3f);
	for (int k = 0; k < n; ++k) {
		float pk;
		const djb::vec3 fk = abc.evalp_pdf_proxy(ggx, i[k], o[k], &pk, NULL, &pg);
		show("abc_ggx_scalar", fk, pk);
	}
	abc.evalp_pdf_proxy(ggx, (size_t)n, &i[0], &o[0], &fr[0], &pdf[0], NULL, &pg);
	for (int k = 0; k < n; ++k) show("abc_ggx_batch", fr[k], pdf[k]);
	for (int k = 0; k < n; ++k) {
		float pk;
		const djb::vec3 fk = sgd.evalp_pdf_proxy(beckmann, i[k], o[k], &pk, NULL, &pb);
		show("sgd_beckmann_scalar", fk, pk);
	}
	sgd.evalp_pdf_proxy(beckmann, (size_t)n, &i[0], &o[0], &fr[0], &pdf[0], NULL, &pb);
	for (int k = 0; k < n; ++k) show("sgd_beckmann_batch", fr[k], pdf[k]);
	return 0;
}
