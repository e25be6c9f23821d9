// tests/hostcheck/bufferrangescheck.cpp -- TEST HARNESS ONLY.
// Drives the real buffer-range rules (cuda-sfm_amd/csrc/buffer_ranges.hpp) and the job order of a batched launch
// (cuda-sfm_amd/csrc/job_order.hpp) from tests/test_buffer_ranges_host.py.  Built by the plain host compiler: neither header
// includes a HIP header.  Nothing in the product loads this library.
#include "../../cuda-sfm_amd/csrc/buffer_ranges.hpp"
#include "../../cuda-sfm_amd/csrc/job_order.hpp"

using namespace sfm;

// range i of the arrays, named by its own index: name = names + i
static std::vector<BufferRange> ranges_of(const uint64_t *addr, const uint64_t *bytes, const int *out, const int *owner, int n, const char *names)
{
    std::vector<BufferRange> r((size_t)n);
    for (int i = 0; i < n; ++i) r[(size_t)i] = { reinterpret_cast<const void *>((uintptr_t)addr[i]), (size_t)bytes[i], out[i] != 0, owner[i], names + i };
    return r;
}

static int answer(const RangeConflict &c, const char *names, int *a, int *b)
{
    if (!c) return 0;
    *a = (int)(c.a->name - names); *b = (int)(c.b->name - names);
    return 1;
}

extern "C" {

// 1 and the indices of the two ranges (a: the output, b: what it lies on), or 0
int br_first_in_set(const uint64_t *addr, const uint64_t *bytes, const int *out, const int *owner, int n, int *a, int *b)
{
    const std::vector<char> names((size_t)n + 1);
    const std::vector<BufferRange> r = ranges_of(addr, bytes, out, owner, n, names.data());
    return answer(first_conflict_in_set(r.data(), r.size()), names.data(), a, b);
}

// 1 and the indices of the two ranges, or 0
int br_first_across_owners(const uint64_t *addr, const uint64_t *bytes, const int *out, const int *owner, int n, int *a, int *b)
{
    const std::vector<char> names((size_t)n + 1);
    std::vector<BufferRange> r = ranges_of(addr, bytes, out, owner, n, names.data());
    return answer(first_conflict_across_owners(r), names.data(), a, b);
}

uint64_t br_bytes_until_known(int n, uint64_t per_record) { return (uint64_t)bytes_until_known(n, (size_t)per_record); }

void jo_order(const int *keys, int count, int *order)
{
    const std::vector<int> o = order_by_decreasing_key(count, [keys](int i) { return keys[i]; });
    for (int k = 0; k < count; ++k) order[k] = o[(size_t)k];
}

}
