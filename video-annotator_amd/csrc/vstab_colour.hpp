// vstab_colour.hpp -- a colour spec (matrix, range) on the host: its check and its coefficient block (vstab_colour.cpp).
#pragma once
#include "vstab_device.hpp"
#include "vstab_internal.hpp"

namespace vstab {

inline bool colour_spec_default(int matrix, int range) { return matrix == VSTAB_COLOUR_CVTCOLOR && range == VSTAB_RANGE_LIMITED; }
bool colour_spec_valid(int matrix, int range);
// refuses an unknown matrix, an unknown range and (CVTCOLOR, FULL) with VSTAB_ERR_INVALID under the caller's name n
vstab_status check_colour_spec(const char *n, int matrix, int range);
// the block of a valid spec, in vstab_colour_coefficients' order
ColourCoef colour_coefficients(int matrix, int range);
// the 10-bit path's block of the same spec, in vstab_colour_coefficients10's order ("Colour matrix and range at 10 bits")
ColourCoef colour_coefficients10(int matrix, int range);

}  // namespace vstab
