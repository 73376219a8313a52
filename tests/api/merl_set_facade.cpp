// merl_set_facade.cpp -- djb::merl_set of the djb:: facade (include/djb_hip.hpp): a set of the two MERL files named on the command line,
// evalp and evalp_is_proxy of five hits (one of them inactive); prints every unit as hex floats.  tests/test_merl_set_host.py runs it
// on the CPU context (DJB_DEVICE=cpu) and holds the lines against the Python mirror's results for the same inputs.
#include <cstdio>
#include <vector>
#include "dj_brdf.h"

int main(int argc, char **argv)
{
	if (argc < 3) return 2;
	const int n = 5;
	const int32_t ids[n] = { 0, 1, -1, 1, 0 };
	const float u1[n] = { 0.1f, 0.35f, 0.5f, 0.75f, 0.9f }, u2[n] = { 0.8f, 0.6f, 0.45f, 0.2f, 0.05f };
	const float dir[n][3] = { { 0.1f, 0.3f, 0.9486833f }, { 0.3f, 0.2f, 0.9327379f }, { 0.5f, 0.1f, 0.8602325f }, { 0.7f, 0.0f, 0.7141428f },
	                          { 0.9f, -0.1f, 0.4242641f } };
	std::vector<djb::vec3> o(n), in(n), w(n), i(n);
	std::vector<float> pdf(n);
	for (int k = 0; k < n; ++k) { o[k] = djb::vec3(dir[k][0], dir[k][1], dir[k][2]); in[k] = djb::vec3(dir[n - 1 - k][1], dir[n - 1 - k][0], dir[n - 1 - k][2]); }
	const djb::microfacet::params pp[2] = { djb::microfacet::params::isotropic(0.3f), djb::microfacet::params::elliptic(0.2f, 0.5f, 0.7f) };
	djb::merl_set *set;
	{
		djb::merl a(argv[1]), b(argv[2]);
		const djb::merl *members[2] = { &a, &b };
		set = new djb::merl_set(2, members);            // the members go out of scope: the set holds copies of their tables
	}
	if (set->size() != 2 || set->has_proxy_params()) return 3;
	set->set_proxy_params(pp);
	if (!set->has_proxy_params()) return 4;
	set->evalp((size_t)n, ids, &in[0], &o[0], &w[0]);
	for (int k = 0; k < n; ++k) printf("evalp %a %a %a\n", w[k].x, w[k].y, w[k].z);
	djb::ggx ggx;
	set->evalp_is_proxy(ggx, (size_t)n, ids, u1, u2, &o[0], &w[0], &i[0], &pdf[0]);
	for (int k = 0; k < n; ++k) printf("sample %a %a %a %a %a %a %a\n", w[k].x, w[k].y, w[k].z, i[k].x, i[k].y, i[k].z, pdf[k]);
	delete set;
	return 0;
}
