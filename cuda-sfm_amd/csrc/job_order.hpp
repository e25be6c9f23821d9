// job_order.hpp -- the order of the jobs of a batched call (common.hpp: job_array_stage).  No HIP header: a host compiler builds
// this file alone (tests/hostcheck/bufferrangescheck.cpp).
#pragma once
#include <algorithm>
#include <vector>

namespace sfm {

// The caller's indices 0 .. count-1 by decreasing key(i): the largest job first, because the one-block chains of a launch are
// dispatched in job order.  Stable, so equal keys keep the caller's order; a job's result does not depend on its place (every
// block works on its own job's buffers).
template <typename Key>
inline std::vector<int> order_by_decreasing_key(int count, Key key)
{
    std::vector<int> order((size_t)(count > 0 ? count : 0));
    for (int i = 0; i < count; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key(x) > key(y); });
    return order;
}

} // namespace sfm
