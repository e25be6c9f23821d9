// TEST SUPPORT: the row a ring entry of the paired passes decides on (prefilter_math.hpp: pf_ring_row, kPfTagScan), host-compiled for
// tests/test_pf_ring_carry_host.py.  The scoring kernel's flush calls the same helper on the entry's tag.
#include <cstdint>
#include "../../cuda-sfm_amd/csrc/prefilter_math.hpp"

extern "C" {

// the table's entry for the survivor at bit (31 - b) of an entry's mask: row offset | step << 5
unsigned pfring_pack_code(int b) { return sfm::pf_pack_code(b); }

// the tag a lane appends: the LDS byte address of its point (a multiple of 16) + 4 (lane >> 5) + (two-step index << 10), and the scan
// bit from the second scan of a pair on -- as ransac_prefilter.hip builds lane_tag
unsigned pfring_tag(unsigned point_address, int half, int pp, int scan)
{
    unsigned tag = point_address + 4u * (unsigned)half + ((unsigned)pp << 10);
    if (scan) tag |= sfm::kPfTagScan;
    return tag;
}

// what the flush reads the point through
unsigned pfring_tag_address(unsigned tag) { return tag & ~15u; }

// the row among the 64 of a pair's table
int pfring_row(int b, unsigned tag) { return sfm::pf_ring_row(sfm::pf_pack_code(b), tag); }

// the same through the 128-byte table the kernel's flush reads (pf_ring_lut_index into pf_ring_lut_entry): row | step << 8, or -1 for an
// index beyond the table
int pfring_lut_row_step(int b, unsigned tag)
{
    const unsigned i = sfm::pf_ring_lut_index(b, tag);
    if (i >= (unsigned)sfm::kPfRingLutBytes) return -1;
    const unsigned e = sfm::pf_ring_lut_entry(i);
    return e < 256u ? (int)((e & 63u) | ((e >> 6) << 8)) : -1;          // (an entry is stored as one byte)
}

// is the survivor counted?  carried ring: the entry's own row against the unit's hypotheses
int pfring_admits(int b, unsigned tag, int nvalid_unit) { return sfm::pf_ring_row(sfm::pf_pack_code(b), tag) < nvalid_unit ? 1 : 0; }

// round 11's test, for an entry flushed during scan `scan` of the unit: the half's row against the scan's (hoff, nvalid); writes the
// table row it would count into
int pfring_admits_scanwise(int b, unsigned tag, int nvalid_unit, int scan, int *row)
{
    const int hoff = scan ? 32 : 0;
    const int nvalid = scan ? nvalid_unit - 32 : (nvalid_unit < 32 ? nvalid_unit : 32);
    const int hl = (int)(sfm::pf_pack_code(b) & 31u) + (int)(tag & 4u);
    *row = hl + hoff;
    return hl < nvalid ? 1 : 0;
}

}
