"""The packed scan's survivor decode without its table (csrc/prefilter_math.hpp: pf_pack_code_closed, what the scoring kernel's
flush runs) against the table it replaces (pf_pack_code) and against the layout the table stands for -- through the host program
tests/hostcheck/pfdecodecheck (make hostcheck).  The header proves the same equality at compile time; this is the run-time twin and
the walk over whole survivor masks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "tests", "hostcheck", "pfdecodecheck")


def run_check():
    assert os.path.exists(PROG), f"{PROG} is missing: make hostcheck builds it"
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout.split("\n")


def expected_code(b):
    """Bit 31 - b of the merged word, from the layout alone: the conversion writes accumulator j of step s as field f = 2 j + s, its
    reject bit at bit 6 f + 4 of 192; registers 0..2 go to the even bits of the word (bit p of register r stays at p), registers
    3..5 to the odd bits (shifted up by one).  Code = MFMA row offset (j & 3) + 8 (j >> 2) | s << 5."""
    pos = 31 - b
    for f in range(32):
        bit = 6 * f + 4
        reg, p = bit // 32, bit % 32
        if (p if reg < 3 else p + 1) == pos and (reg >= 3) == bool(pos & 1):
            j, s = f >> 1, f & 1
            return ((j & 3) + 8 * (j >> 2)) | (s << 5)
    raise AssertionError(f"no field lands on bit {pos}")


def test_closed_form_equals_the_table_for_every_position():
    rc, lines = run_check()
    rows = [tuple(int(v) for v in ln.split()) for ln in lines[:32]]
    assert [r[0] for r in rows] == list(range(32))
    for b, closed, table in rows:
        assert closed == table == expected_code(b), (b, closed, table, expected_code(b))
    assert sorted(r[1] for r in rows) == sorted(((j & 3) + 8 * (j >> 2)) | (s << 5) for j in range(16) for s in range(2)), "not a permutation"
    assert rc == 0


def test_mask_walks_visit_the_same_rows_and_steps():
    """Every survivor mask with one, two or three bits set: clz -> decode -> clear gives the same (row, step) sequence either way."""
    rc, lines = run_check()
    tail = [ln for ln in lines if ln.startswith("walks")]
    assert len(tail) == 1
    _, masks, _, mismatches = tail[0].split()
    assert int(masks) == 32 + 32 * 31 // 2 + 32 * 31 * 30 // 6
    assert int(mismatches) == 0 and rc == 0


def test_which_launches_sum_their_counts():
    """The launcher's own size rule (prefilter_lds.hpp: pf_sums_counts_at), asked through the host program: counts are summed without
    an answer from 2^21 (hypothesis, tile) partial counts per launch on.  A pair's row length is its point count rounded up to 128."""
    def sums(count, n):
        ld = (n + 127) // 128 * 128
        r = subprocess.run([PROG, "sums", str(count), str(ld)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0
        w = r.stdout.split()
        return int(w[1]), int(w[3]), bool(int(w[5]))
    assert sums(1 << 20, 4096) == (1024, 4, True)                  # the headline
    assert sums(1 << 19, 4096) == (1024, 4, True)                  # 2^21 exactly
    assert sums((1 << 19) - 1, 4096) == (1024, 4, False)
    assert sums(131072, 4096)[2] is False                          # a rank's share of the headline
    assert sums(65536, 16384) == (1024, 16, False)                 # configs[2]: 2^20 partial counts
    assert sums(1 << 20, 16384) == (1024, 16, True)                # configs[3]
    assert sums(1 << 20, 1025) == (576, 2, True) and sums((1 << 20) - 1, 1025) == (576, 2, False)      # tests/test_gpu_pass_tail.py
    assert sums(33, 96)[2] is False
