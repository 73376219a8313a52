// merl_set_light_facade.cpp -- djb::merl_set::evalp_pdf_proxy of the djb:: facade (include/djb_hip.hpp): a set of the two MERL files named
// on the command line, the light sample of five given pairs -- one inactive, one with i.z < 0, one with o.z < 0 -- against a ggx and a
// beckmann proxy; prints every unit as hex floats.  tests/test_merl_set_light_host.py runs it on the CPU context (DJB_DEVICE=cpu) and
// holds the lines against the Python mirror's results for the same inputs.
#include <cstdio>
#include <vector>
#include "dj_brdf.h"

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	const int n = 5;
	const int32_t ids[n] = { 0, 1, -1, 1, 0 };
	const float od[n][3] = { { 0.1f, 0.3f, 0.9486833f }, { 0.3f, 0.2f, 0.9327379f }, { 0.5f, 0.1f, 0.8602325f }, { 0.7f, 0.0f, 0.7141428f },
	                         { 0.9f, -0.1f, -0.4242641f } };
	const float id[n][3] = { { -0.1f, -0.25f, 0.9630680f }, { -0.3f, -0.2f, -0.9327379f }, { 0.1f, 0.5f, 0.8602325f }, { -0.6f, 0.1f, 0.7937254f },
	                         { 0.2f, 0.2f, 0.9591663f } };
	std::vector<djb::vec3> o(n), i(n), fr(n);
	std::vector<float> pdf(n);
	for (int k = 0; k < n; ++k) { o[k] = djb::vec3(od[k][0], od[k][1], od[k][2]); i[k] = djb::vec3(id[k][0], id[k][1], id[k][2]); }
	const djb::microfacet::params pp[2] = { djb::microfacet::params::isotropic(0.3f), djb::microfacet::params::elliptic(0.2f, 0.5f, 0.7f) };
	djb::merl a(argv[1]), b(argv[2]);
	const djb::merl *members[2] = { &a, &b };
	djb::merl_set set(2, members, pp);
	djb::ggx ggx;
	set.evalp_pdf_proxy(ggx, (size_t)n, ids, &i[0], &o[0], &fr[0], &pdf[0]);
	for (int k = 0; k < n; ++k) printf("ggx %a %a %a %a\n", fr[k].x, fr[k].y, fr[k].z, pdf[k]);
	djb::beckmann beckmann;
	set.evalp_pdf_proxy(beckmann, (size_t)n, ids, &i[0], &o[0], &fr[0], &pdf[0]);
	for (int k = 0; k < n; ++k) printf("beckmann %a %a %a %a\n", fr[k].x, fr[k].y, fr[k].z, pdf[k]);
	return 0;
}
