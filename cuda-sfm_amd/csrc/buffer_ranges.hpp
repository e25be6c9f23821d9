// buffer_ranges.hpp -- THE rule about the caller's buffers of a call whose blocks run at the same time: no output on an input or on
// another output.  One range type, the rule inside one set (a single call, one entry of a batched call), the rule
// across the sets of a batched call, and how long an array counts before its pair has been looked at.  No HIP header: a host
// compiler builds this file alone (tests/hostcheck/bufferrangescheck.cpp).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

namespace sfm {

// owner: the list entry (pair, link) whose blocks touch the range; name: what a message calls it
struct BufferRange { const void *p; size_t bytes; bool out; int owner; const char *name; };
struct RangeConflict { const BufferRange *a = nullptr, *b = nullptr; explicit operator bool() const { return a != nullptr; } };

// An array of n records counts as ONE byte until the pair has been looked at (n == 0): the same address is caught before any
// pair is dereferenced, and anything inside a buffer of fixed size.
inline size_t bytes_until_known(int n, size_t per_record) { return n ? (size_t)n * per_record : (size_t)1; }

// a null pointer and an empty range lie on nothing; ranges that only touch do not overlap
inline bool ranges_overlap(const BufferRange &x, const BufferRange &y)
{
    if (!x.p || !y.p || !x.bytes || !y.bytes) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(x.p), b = reinterpret_cast<uintptr_t>(y.p);
    return a < b + y.bytes && b < a + x.bytes;
}

// Inside one set, whatever the owners: the outputs in the order of the list, each against every input and then against the
// outputs after it.  Returns the first such pair (a: the output, b: what it lies on), so a message names the same two buffers
// whatever else is wrong.  Quadratic: a set has about ten ranges.
inline RangeConflict first_conflict_in_set(const BufferRange *r, size_t count)
{
    RangeConflict c;
    for (size_t o = 0; o < count; ++o) {
        if (!r[o].out) continue;
        for (size_t i = 0; i < count; ++i) if (!r[i].out && ranges_overlap(r[o], r[i])) { c.a = &r[o]; c.b = &r[i]; return c; }
        for (size_t q = o + 1; q < count; ++q) if (r[q].out && ranges_overlap(r[o], r[q])) { c.a = &r[o]; c.b = &r[q]; return c; }
    }
    return c;
}

// Across owners: two ranges of DIFFERENT owners that overlap, at least one of them an output (inputs may be shared), or nothing.
// All ranges sorted by their start (r is reordered; null and empty ranges are dropped), one sweep that keeps the range seen so
// far that ends last -- any, and among the outputs: an output is held against the first, an input against the second.
// PRECONDITION: no conflict inside one owner (first_conflict_in_set over every owner's ranges found nothing).  A hit on the
// range that ends last is skipped when it has the same owner, and a range of another owner behind it is then not looked at:
// inputs [0,100) of owner 0 and [10,50) of owner 1 with the output [20,30) of owner 0 pass the sweep, and only the rule
// inside owner 0 refuses them.  With it the skip loses nothing: an output never lies on a range of its own owner, so the range
// that ends last is of another owner whenever anything reaches the output.  Callers that give every range its own owner
// (sfm_fuse_chain) have nothing to exempt and need no other check.
// a: the range that starts later (or sorts later), b: the earlier one it reaches into.
inline RangeConflict first_conflict_across_owners(std::vector<BufferRange> &r)
{
    r.erase(std::remove_if(r.begin(), r.end(), [](const BufferRange &x) { return !x.p || !x.bytes; }), r.end());
    std::sort(r.begin(), r.end(), [](const BufferRange &x, const BufferRange &y) { return reinterpret_cast<uintptr_t>(x.p) < reinterpret_cast<uintptr_t>(y.p); });
    auto end = [](const BufferRange &x) { return reinterpret_cast<uintptr_t>(x.p) + x.bytes; };
    RangeConflict c;
    const BufferRange *far_any = nullptr, *far_out = nullptr;
    for (const BufferRange &x : r) {
        const BufferRange *hit = x.out ? far_any : far_out;
        if (hit && end(*hit) > reinterpret_cast<uintptr_t>(x.p) && hit->owner != x.owner) { c.a = &x; c.b = hit; return c; }
        if (!far_any || end(x) > end(*far_any)) far_any = &x;
        if (x.out && (!far_out || end(x) > end(*far_out))) far_out = &x;
    }
    return c;
}

// The same rule for a call whose owners MAY overlap themselves (sfm_match_guided_pairs: a job may match a set against itself,
// as the single call may): no precondition.  The sweep keeps, among all ranges seen and among the outputs, the range that ends
// last AND the one that ends last among the other owners' -- whichever owner x has, the farthest-reaching range of another owner
// is one of the two, so a range of x's own owner in front never hides one behind it.
inline RangeConflict first_conflict_across_overlapping_owners(std::vector<BufferRange> &r)
{
    r.erase(std::remove_if(r.begin(), r.end(), [](const BufferRange &x) { return !x.p || !x.bytes; }), r.end());
    std::sort(r.begin(), r.end(), [](const BufferRange &x, const BufferRange &y) { return reinterpret_cast<uintptr_t>(x.p) < reinterpret_cast<uintptr_t>(y.p); });
    auto end = [](const BufferRange &x) { return reinterpret_cast<uintptr_t>(x.p) + x.bytes; };
    struct Far {
        const BufferRange *first = nullptr, *other = nullptr;          // ends last; ends last among the owners that are not first's
    };
    auto keep = [&end](Far &f, const BufferRange &x) {
        if (!f.first) { f.first = &x; return; }
        if (x.owner == f.first->owner) { if (end(x) > end(*f.first)) f.first = &x; return; }
        if (end(x) > end(*f.first)) { f.other = f.first; f.first = &x; return; }
        if (!f.other || end(x) > end(*f.other)) f.other = &x;
    };
    RangeConflict c;
    Far any, out;
    for (const BufferRange &x : r) {
        const Far &f = x.out ? any : out;
        const BufferRange *hit = f.first && f.first->owner != x.owner ? f.first : f.other;
        if (hit && hit->owner != x.owner && end(*hit) > reinterpret_cast<uintptr_t>(x.p)) { c.a = &x; c.b = hit; return c; }
        keep(any, x);
        if (x.out) keep(out, x);
    }
    return c;
}

} // namespace sfm
