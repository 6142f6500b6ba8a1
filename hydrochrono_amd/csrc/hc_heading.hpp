// hc_heading.hpp -- the bracket rule of a heading grid, shared by the first-order excitation under a heading (hc_directions.cpp) and
// the QTF tables on a heading grid (hc_qtf.hip).  Host code.
#pragma once
#include "hc_internal.hpp"

#include <algorithm>
#include <vector>

namespace hc {
namespace detail {

// The two grid headings around theta and the weight of the second: the largest j0 with dir[j0] <= theta, so that a theta on a grid
// node has weight exactly 0 and the node's table comes out bit for bit.  No extrapolation, no wrap-around: a theta outside the grid
// fails with HC_ERR_INVALID and `outside`, the caller's words for its grid.
struct HeadBracket {
    int j0, j1;
    double wt;
};
inline HeadBracket heading_bracket(const std::vector<double>& dir, double theta, const char* outside) {
    require(theta >= dir.front() && theta <= dir.back(), HC_ERR_INVALID, outside);
    const int n  = static_cast<int>(dir.size());
    const int j0 = static_cast<int>(std::upper_bound(dir.begin(), dir.end(), theta) - dir.begin()) - 1;
    if (j0 >= n - 1) return HeadBracket{n - 1, n - 1, 0.0};
    return HeadBracket{j0, j0 + 1, (theta - dir[j0]) / (dir[j0 + 1] - dir[j0])};
}

}  // namespace detail
}  // namespace hc
