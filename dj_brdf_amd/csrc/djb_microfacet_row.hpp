// djb_microfacet_row.hpp -- one material of a microfacet set (include/djb_hip.h: djb_microfacet_set), as the set keeps it resident and as
// the kernels (djb_kernels_microfacet_set.hip) and the host loops (djb_cpu.cpp: LobeMat) read it.  Included after djb_device.hpp.
#pragma once

namespace djbdev {

// The resolved parameter set exactly as the single-material call hands it to its kernel (r_ax / r_t2 included; 0 on a CPU context, whose
// fdiv_r divides), then what the call takes from its object: the Fresnel term (kind, a[3], b[3]; no spline: its point list has no fixed
// size) and the shadowing flag.  88 bytes = 11 eight-byte units: an ODD number, see djb_kernels_microfacet_set.hip for the LDS banks.
struct MfRow {
	Params p;
	int fr_kind;
	float a[3], b[3];
	int shadow;
};
constexpr int MF_ROW_BYTES = 88;
static_assert(sizeof(MfRow) == MF_ROW_BYTES && alignof(MfRow) == 8, "MfRow: 56 bytes of Params, 32 of Fresnel term and flag");

} // namespace djbdev
