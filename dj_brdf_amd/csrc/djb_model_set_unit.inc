// djb_model_set_unit.inc -- what the kernels of an SGD / ABC model set share (djb_kernels_model_set.hip, djb_kernels_model_set_proxy.hip):
// the layout of a resident row and the evaluation of one active hit on it.  Included inside each file's anonymous namespace, after
// `using namespace djbdev`.
constexpr int row_stride(int kind) { return kind == KIND_SGD ? (int)SGD_FAST_ROW : 9; }                 // doubles per resident row

// one active hit: the hit's row becomes the lane's Brdf -- `model` and the Fresnel operands create_model derives from the row
template <int KIND, int WANT>
DJB_DEV void unit(Brdf b, const double *m, v3 i, v3 o, v3 &fr)
{
	b.model = m;
	b.fr.kind = KIND == KIND_SGD ? FR_SGD : FR_UNPOLARIZED;      // a compile-time constant here: fresnel_eval's switch folds to the kind's term
	if (KIND == KIND_SGD) {
#pragma unroll
		for (int c = 0; c < 3; ++c) { b.fr.a[c] = (float)m[12 + c]; b.fr.b[c] = (float)m[15 + c]; }
	} else b.fr.a[0] = b.fr.a[1] = b.fr.a[2] = (float)m[8];
	const Params none = {};
	float pdf = 0.0f;
	eval_one<KIND, WANT>(b, none, i, o, fr, pdf);
}
