// vstab_colour.cpp -- the coefficient table of a colour spec (include/vstab.h, "Colour matrix and range"): host only, no device needed.
// The cvtColor row is read from the constant types of vstab_device.hpp (CvtColor8 / CvtColor10), which the default kernels are compiled
// with; the other six are derived here from (Kr, Kb) and the range in exact integer rational arithmetic, rounded half to even.
#include "vstab_colour.hpp"

namespace vstab {

namespace {

// round(n / d) half to even, d > 0
int64_t rint_ratio(int64_t n, int64_t d) {
    int64_t q = n / d, r = n % d;
    if (r < 0) q--, r += d;  // floor
    if (2 * r > d || (2 * r == d && (q & 1))) q++;
    return q;
}

}  // namespace

bool colour_spec_valid(int matrix, int range) {
    if (matrix < VSTAB_COLOUR_CVTCOLOR || matrix > VSTAB_COLOUR_BT2020) return false;
    if (range != VSTAB_RANGE_LIMITED && range != VSTAB_RANGE_FULL) return false;
    return !(matrix == VSTAB_COLOUR_CVTCOLOR && range == VSTAB_RANGE_FULL);
}

// The six derived rows at either depth: sy = yn / yd, sc = cn / cd and the luma offset are what the depth and the range decide.
// Kr = kr / D, Kb = kb / D, Kg = kg / D.  The largest product below, 2^21 * 1023 * D * D, is 2.2e17.
static ColourCoef derive(int matrix, int64_t yn, int64_t yd, int64_t cn, int64_t cd, int yoff) {
    const int64_t D = 10000, one = 1 << 20;
    const int64_t kr = matrix == VSTAB_COLOUR_BT601 ? 2990 : matrix == VSTAB_COLOUR_BT709 ? 2126 : 2627;
    const int64_t kb = matrix == VSTAB_COLOUR_BT601 ? 1140 : matrix == VSTAB_COLOUR_BT709 ? 722 : 593;
    const int64_t kg = D - kr - kb;
    ColourCoef c;
    c.cy = (int)rint_ratio(one * yn, yd);
    c.cvr = (int)rint_ratio(one * cn * 2 * (D - kr), cd * D);
    c.cub = (int)rint_ratio(one * cn * 2 * (D - kb), cd * D);
    c.cug = -(int)rint_ratio(one * cn * 2 * kb * (D - kb), cd * D * kg);
    c.cvg = -(int)rint_ratio(one * cn * 2 * kr * (D - kr), cd * D * kg);
    c.yoff = yoff;
    c.cry = (int)rint_ratio(one * kr * yd, D * yn);
    c.cgy = (int)rint_ratio(one * kg * yd, D * yn);
    c.cby = (int)rint_ratio(one * kb * yd, D * yn);
    c.cbu = (int)rint_ratio(one * cd, 2 * cn);
    c.cru = -(int)rint_ratio(one * kr * cd, 2 * (D - kb) * cn);
    c.cgu = -(int)rint_ratio(one * kg * cd, 2 * (D - kb) * cn);
    c.cgv = -(int)rint_ratio(one * kg * cd, 2 * (D - kr) * cn);
    c.cbv = -(int)rint_ratio(one * kb * cd, 2 * (D - kr) * cn);
    return c;
}

// cvtColor's row: the constants the default kernels are compiled with, K = CvtColor8 or CvtColor10
template <typename K>
static ColourCoef cvtcolor_row() {
    return {K::cy, K::cub, K::cug, K::cvg, K::cvr, K::yoff, K::cry, K::cgy, K::cby, K::cru, K::cgu, K::cbu, K::cgv, K::cbv};
}

ColourCoef colour_coefficients(int matrix, int range) {
    if (matrix == VSTAB_COLOUR_CVTCOLOR) return cvtcolor_row<CvtColor8>();
    if (range == VSTAB_RANGE_FULL) return derive(matrix, 1, 1, 1, 1, 0);
    return derive(matrix, 255, 219, 255, 224, 16);
}

// The 10-bit table (include/vstab.h, "Colour matrix and range at 10 bits"): cvtColor's row with the luma offset of 10-bit video, which is the
// 10-bit path's arithmetic as it always was; the other six with the 10-bit scales 1023/876 and 1023/896.
ColourCoef colour_coefficients10(int matrix, int range) {
    if (matrix == VSTAB_COLOUR_CVTCOLOR) return cvtcolor_row<CvtColor10>();
    if (range == VSTAB_RANGE_FULL) return derive(matrix, 1, 1, 1, 1, 0);
    return derive(matrix, 1023, 876, 1023, 896, 64);
}

vstab_status check_colour_spec(const char *n, int matrix, int range) {
    if (matrix < VSTAB_COLOUR_CVTCOLOR || matrix > VSTAB_COLOUR_BT2020)
        return fail(VSTAB_ERR_INVALID, std::string(n) + ": matrix must be VSTAB_COLOUR_CVTCOLOR (0), _BT601 (1), _BT709 (2) or _BT2020 (3)");
    if (range != VSTAB_RANGE_LIMITED && range != VSTAB_RANGE_FULL)
        return fail(VSTAB_ERR_INVALID, std::string(n) + ": range must be VSTAB_RANGE_LIMITED (0) or VSTAB_RANGE_FULL (1)");
    if (matrix == VSTAB_COLOUR_CVTCOLOR && range == VSTAB_RANGE_FULL)
        return fail(VSTAB_ERR_INVALID, std::string(n) + ": VSTAB_COLOUR_CVTCOLOR is cvtColor's limited-range arithmetic; full range needs a matrix (BT601, BT709, BT2020)");
    return VSTAB_OK;
}

}  // namespace vstab

using namespace vstab;

static vstab_status write_coefficients(const char *n, int matrix, int range, bool ten, int32_t out[14]) {
    if (!out) return fail(VSTAB_ERR_INVALID, std::string(n) + ": null pointer");
    VSTAB_TRY(check_colour_spec(n, matrix, range));
    const ColourCoef c = ten ? colour_coefficients10(matrix, range) : colour_coefficients(matrix, range);
    const int v[14] = {c.cy, c.cub, c.cug, c.cvg, c.cvr, c.yoff, c.cry, c.cgy, c.cby, c.cru, c.cgu, c.cbu, c.cgv, c.cbv};
    for (int i = 0; i < 14; i++) out[i] = v[i];
    return VSTAB_OK;
}

extern "C" vstab_status vstab_colour_coefficients(int matrix, int range, int32_t out[14]) {
    return write_coefficients("vstab_colour_coefficients", matrix, range, false, out);
}

extern "C" vstab_status vstab_colour_coefficients10(int matrix, int range, int32_t out[14]) {
    return write_coefficients("vstab_colour_coefficients10", matrix, range, true, out);
}
