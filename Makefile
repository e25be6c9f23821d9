# Builds the MI355X-native library (hand-written HIP for gfx950 behind the C ABI in include/),
# the CPU oracle (test infrastructure) and the host-compiled arithmetic check used by CPU tests.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
# -ffp-contract=off + correctly rounded div/sqrt: the arithmetic contract shared with oracle/
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -DOCML_BASIC_ROUNDED_OPERATIONS \
            -fPIC -fvisibility=hidden -Wall -Wno-unused-function -Wno-pass-failed
PKG      := cuda-sfm_amd
CSRC     := $(PKG)/csrc
BUILD    := build
BUILD_AB := build/ab
LIB      := $(PKG)/lib/libsfm_amd.so
COMMLIB  := $(PKG)/lib/libsfm_amd_rccl.so
# Two flavours of the same sources:
#   libsfm_amd.so     the product: what include/sfm_amd.h declares, nothing else (sfm_ransac_params.reserved[] must be 0)
#   libsfm_amd_ab.so  the lab bench (-DSFM_AB=1): + the A/B switches behind reserved[], the recorded slower kernel variants
#                     ($(CSRC)/ab/*.hip) and the probe / trace hooks of include/sfm_amd_ab.h.  Loaded only by tests/ and
#                     profiles/ (`import cuda_sfm_amd_ab`), never by the product path.
LIB_AB   := $(PKG)/lib/libsfm_amd_ab.so
SRCS     := $(wildcard $(CSRC)/*.hip)
SRCS_AB  := $(wildcard $(CSRC)/ab/*.hip)
OBJS     := $(patsubst $(CSRC)/%.hip,$(BUILD)/%.o,$(SRCS))
OBJS_AB  := $(patsubst $(CSRC)/%.hip,$(BUILD_AB)/%.o,$(SRCS)) $(patsubst $(CSRC)/ab/%.hip,$(BUILD_AB)/ab_%.o,$(SRCS_AB))
HDRS     := $(wildcard $(CSRC)/*.hpp) $(wildcard $(CSRC)/*.inc) include/sfm_amd.h include/sfm_amd_ab.h

DEMO     := $(PKG)/host/two_view_demo
HDEMO    := $(PKG)/host/homography_demo
SDEMO    := $(PKG)/host/sift_demo
MAINAPP  := $(PKG)/host/sfm_main
RPDEMO   := $(PKG)/host/refine_pairs_demo
RVDEMO   := $(PKG)/host/register_views_demo
APDEMO   := $(PKG)/host/align_pairs_demo
FCDEMO   := $(PKG)/host/fuse_chain_demo
GMDEMO   := $(PKG)/host/guided_match_demo
GPDEMO   := $(PKG)/host/guided_pairs_demo

IOTEST   := tests/cpp/io_test
GEOMTEST := tests/cpp/geom_test

all: $(LIB) $(LIB_AB) $(COMMLIB) $(BUILD)/ransac.s $(BUILD)/view_points.s oracle hostcheck fakeccl $(DEMO) $(HDEMO) $(SDEMO) $(MAINAPP) $(RPDEMO) $(RVDEMO) $(APDEMO) $(FCDEMO) $(GMDEMO) $(GPDEMO) $(IOTEST) $(GEOMTEST)

# the product's objects come with the compiler's resource-usage report (registers, scratch, LDS of every kernel) next to them:
# $(BUILD)/<source>.usage.txt, read by tests/test_register_budget.py; warnings and errors of the compile are still shown
$(BUILD)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(FLAGS_$*) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/$*.usage.txt || { cat $(BUILD)/$*.usage.txt >&2; exit 1; }
	@grep -v -e 'remark:' -e '^ *[0-9]* | ' -e '^ *| ' $(BUILD)/$*.usage.txt >&2 || true

# the instruction text of ransac.hip's kernels as the product compiles them (the object's flags, assembly out): the lane-solve kernels'
# issue budget is read from it (tests/test_solve_issue_budget.py, profiles/isa_census.py)
$(BUILD)/ransac.s: $(CSRC)/ransac.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(FLAGS_ransac) --cuda-device-only -S $< -o $@

# the same for view_points.hip: the record loads its source describes are read back from it (tests/test_view_points_host.py)
$(BUILD)/view_points.s: $(CSRC)/view_points.hip $(HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(FLAGS_view_points) --cuda-device-only -S $< -o $@

$(BUILD_AB)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(BUILD_AB)
	$(HIPCC) $(HIPFLAGS) -DSFM_AB=1 $(FLAGS_$*) -c $< -o $@

$(BUILD_AB)/ab_%.o: $(CSRC)/ab/%.hip $(HDRS)
	@mkdir -p $(BUILD_AB)
	$(HIPCC) $(HIPFLAGS) -DSFM_AB=1 -I$(CSRC) -c $< -o $@

# the lane-solve kernels are long chains of scalar FP32 operations: the SLP vectoriser pairs some of them into v_pk_* and pays
# for it with register moves (366 v_mov in 2473 instructions); without it the same arithmetic needs fewer issue slots
FLAGS_ransac := -fno-slp-vectorize
# match_fused's two interleaved exact chains: paired into v_pk_fma_f32 they need a register move per operand
FLAGS_match_fused := -fno-slp-vectorize
# adjust.hip's solve kernel keeps both cameras in scalar registers: paired into v_pk_* the terms need scalar pairs that are moved and
# spilled (256 VGPRs + 672 bytes of scratch with the vectoriser, no scratch without)
FLAGS_adjust := -fno-slp-vectorize
# align.hip's lane solve sits at the 64-register boundary with the vectoriser's register pairs (64 single, 66 batched: 7 waves per
# SIMD instead of 8); without it the four kernels need 52 / 55 / 92 / 250 VGPRs, the batched ones the same as their twins
FLAGS_align := -fno-slp-vectorize

$(LIB): $(OBJS) $(CSRC)/exports.map
	@mkdir -p $(PKG)/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--version-script=$(CSRC)/exports.map -o $@ $(OBJS) -lpthread

$(LIB_AB): $(OBJS_AB) $(CSRC)/exports.map
	@mkdir -p $(PKG)/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--version-script=$(CSRC)/exports.map -o $@ $(OBJS_AB) -lpthread

ab: $(LIB_AB)

# the RCCL exchange step lives in its own library: libsfm_amd.so itself has no RCCL dependency
$(COMMLIB): $(CSRC)/comm.cpp include/sfm_amd_comm.h include/sfm_amd.h $(LIB)
	$(HIPCC) -x hip --cuda-host-only -O2 -fPIC -fvisibility=hidden -shared -Iinclude -Wl,--version-script=$(CSRC)/exports.map -o $@ $< -L$(PKG)/lib -lsfm_amd -L/opt/rocm/lib -lrccl -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,/opt/rocm/lib

oracle:
	$(MAKE) -C oracle

# plain C++ host program on the facade headers: no HIP headers, links only the C-ABI library
$(DEMO): $(PKG)/host/two_view_demo.cpp $(PKG)/host/sfm.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(HDEMO): $(PKG)/host/homography_demo.cpp $(PKG)/host/geomFuncs.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -ffp-contract=off -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(SDEMO): $(PKG)/host/sift_demo.cpp $(PKG)/host/cudaImage.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(MAINAPP): $(PKG)/host/sfm_main.cpp $(PKG)/host/cudaImage.h $(PKG)/host/sfm.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(RPDEMO): $(PKG)/host/refine_pairs_demo.cpp $(PKG)/host/sfm.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(RVDEMO): $(PKG)/host/register_views_demo.cpp $(PKG)/host/sfm.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(APDEMO): $(PKG)/host/align_pairs_demo.cpp $(PKG)/host/sfm.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(FCDEMO): $(PKG)/host/fuse_chain_demo.cpp $(PKG)/host/sfm.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(GMDEMO): $(PKG)/host/guided_match_demo.cpp $(PKG)/host/sfm.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(GPDEMO): $(PKG)/host/guided_pairs_demo.cpp $(PKG)/host/sfm.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h $(LIB)
	g++ -O2 -std=c++14 -Wall -o $@ $< -L$(PKG)/lib -lsfm_amd -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath,/opt/rocm/lib

$(IOTEST): tests/cpp/io_test.cpp $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h
	g++ -O2 -std=c++14 -Wall -o $@ $<

$(GEOMTEST): tests/cpp/geom_test.cpp $(PKG)/host/geomFuncs.h $(PKG)/host/sfm_io.h $(PKG)/host/cudaSift.h include/sfm_amd.h
	g++ -O2 -std=c++14 -ffp-contract=off -Wall -o $@ $<

# CPU-only: the host-compiled arithmetic check of the non-GPU tests (the fakeccl target, which needs the gfx950 build and the RCCL
# header, is a target of its own and part of `all`)
hostcheck: tests/hostcheck/libhostcheck.so tests/hostcheck/librefinecheck.so tests/hostcheck/libregistercheck.so tests/hostcheck/libviewpointscheck.so tests/hostcheck/libadjustcheck.so tests/hostcheck/libaligncheck.so tests/hostcheck/libfusecheck.so tests/hostcheck/libchainadjustcheck.so tests/hostcheck/libringcheck.so tests/hostcheck/libfuseringcheck.so tests/hostcheck/libringadjustcheck.so tests/hostcheck/libintersectcheck.so tests/hostcheck/libpairstatecheck.so tests/hostcheck/libbufferrangescheck.so tests/hostcheck/libpfldscheck.so tests/hostcheck/libpairsplancheck.so tests/hostcheck/pfdecodecheck tests/hostcheck/libpfpaircheck.so tests/hostcheck/libpfringcheck.so tests/hostcheck/libmatchguidedcheck.so tests/hostcheck/libmatchguidedplancheck.so

# TEST HARNESS: comm.cpp linked against a shared-memory stand-in for the nine RCCL calls it makes, so that a 1-GPU box can run the
# exchange code with two real ranks (tests/test_gpu_fakeccl.py); the product's libsfm_amd_rccl.so is linked against librccl
FAKECCL := tests/fake_ccl/libsfm_amd_fakeccl.so
fakeccl: $(FAKECCL)
$(FAKECCL): $(CSRC)/comm.cpp tests/fake_ccl/fake_ccl.cpp include/sfm_amd_comm.h include/sfm_amd.h $(LIB)
	$(HIPCC) -x hip --cuda-host-only -O2 -fPIC -fvisibility=hidden -shared -Iinclude -Wl,--version-script=$(CSRC)/exports.map -o $@ $(CSRC)/comm.cpp tests/fake_ccl/fake_ccl.cpp -L$(PKG)/lib -lsfm_amd -lrt -lpthread -Wl,-rpath,'$$ORIGIN/../../$(PKG)/lib'

tests/hostcheck/libhostcheck.so: tests/hostcheck/hostcheck.hip $(CSRC)/device_math.hpp $(CSRC)/sift_math.hpp $(CSRC)/prefilter_math.hpp $(CSRC)/match_prefilter_math.hpp
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the two-view bundle adjustment's per-point arithmetic (refinecheck.hip), a serial driver of the whole call (refineruncheck.hip:
# rc_run, the fp64 sums in the solve block's order) and the LM control (lmcheck.hip) of refine_math.hpp, host-compiled for
# tests/test_refine_host.py, tests/test_refine_run_host.py, tests/test_lm_control_host.py and the byte comparison of
# tests/test_gpu_refine_host_build.py
tests/hostcheck/librefinecheck.so: tests/hostcheck/refinecheck.hip tests/hostcheck/refineruncheck.hip tests/hostcheck/lmcheck.hip $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ tests/hostcheck/refinecheck.hip tests/hostcheck/refineruncheck.hip tests/hostcheck/lmcheck.hip

# the view registration's arithmetic (register_math.hpp: P3P, sampler, inlier test, pose Jacobian), host-compiled for
# tests/test_register_host.py and the count parity of tests/test_gpu_register.py
tests/hostcheck/libregistercheck.so: tests/hostcheck/registercheck.hip $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_triangulate_view (view_points_math.hpp: DLT start, point LM, acceptance test) run over arrays on the CPU,
# for tests/test_view_points_host.py and the byte parity of tests/test_gpu_view_points.py
tests/hostcheck/libviewpointscheck.so: tests/hostcheck/viewpointscheck.hip $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_adjust_view (adjust_math.hpp: view bits, Jacobians, Schur terms, camera step) and a serial driver of the
# whole chain, for tests/test_adjust_host.py and the comparison of tests/test_gpu_adjust.py
tests/hostcheck/libadjustcheck.so: tests/hostcheck/adjustcheck.hip $(CSRC)/adjust_math.hpp $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_align_pair (align_math.hpp: gate, triad solver, two-way inlier test, Jacobians, step) and a serial driver
# of the whole call, for tests/test_align_host.py and the comparison of tests/test_gpu_align.py
tests/hostcheck/libaligncheck.so: tests/hostcheck/aligncheck.hip $(CSRC)/align_math.hpp $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_fuse_chain (fuse_math.hpp: link validity, frame composition, cameras, edge keys, the point LM over a list
# of views) and a serial driver of the whole call, for tests/test_fuse_host.py and the comparison of tests/test_gpu_fuse.py
tests/hostcheck/libfusecheck.so: tests/hostcheck/fusecheck.hip $(CSRC)/fuse_math.hpp $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_adjust_chain (chain_adjust_math.hpp: block indices, used test, one track's terms over its view list, the
# steps, the banded factor and solve) and a serial driver of the whole call, for tests/test_chain_adjust_host.py and the
# comparison of tests/test_gpu_chain_adjust.py
tests/hostcheck/libchainadjustcheck.so: tests/hostcheck/chainadjustcheck.hip $(CSRC)/chain_adjust_math.hpp $(CSRC)/fuse_math.hpp $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_close_ring (ring_math.hpp: the rotation's logarithm and exponential, the drift and its gates, the weights'
# running sums, the corrected links, the seam test) and a serial driver of the whole call, for tests/test_ring_host.py and the
# comparison of tests/test_gpu_ring.py
tests/hostcheck/libringcheck.so: tests/hostcheck/ringcheck.hip $(CSRC)/ring_math.hpp $(CSRC)/fuse_math.hpp $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_fuse_ring (fuse_ring_math.hpp: the closure and its gates, the walk back to a track's head, the join rule,
# the seam flags) and a serial driver of the whole call, for tests/test_fuse_ring_host.py and the comparison of
# tests/test_gpu_fuse_ring.py
tests/hostcheck/libfuseringcheck.so: tests/hostcheck/fuseringcheck.hip $(CSRC)/fuse_ring_math.hpp $(CSRC)/ring_math.hpp $(CSRC)/fuse_math.hpp $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_adjust_ring (ring_adjust_math.hpp over chain_adjust_math.hpp: the modulo view rule, the reduction of the head
# pairs' partial bands into the folded band, the band claim) and a serial driver of the whole call, for
# tests/test_ring_adjust_host.py and the comparison of tests/test_gpu_ring_adjust.py; the no-scratch pin of ring_adjust.hip reads
# $(BUILD)/ring_adjust.usage.txt, which the object rule above writes
tests/hostcheck/libringadjustcheck.so: tests/hostcheck/ringadjustcheck.hip $(CSRC)/ring_adjust_math.hpp $(CSRC)/chain_adjust_math.hpp $(CSRC)/fuse_math.hpp $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the arithmetic of sfm_intersect_tracks (intersect_math.hpp over fuse_math.hpp: the linear intersection, the eligibility test, the
# start choice, the class mapping) and a serial driver of the whole call that walks every track in list order, for
# tests/test_intersect_host.py and the byte comparison of tests/test_gpu_intersect.py; the no-scratch pin of intersect.hip reads
# $(BUILD)/intersect.usage.txt, which the object rule above writes
tests/hostcheck/libintersectcheck.so: tests/hostcheck/intersectcheck.hip $(CSRC)/intersect_math.hpp $(CSRC)/chain_adjust_math.hpp $(CSRC)/fuse_math.hpp $(CSRC)/view_points_math.hpp $(CSRC)/register_math.hpp $(CSRC)/refine_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the scoring block's dynamic LDS size (prefilter_lds.hpp), host-compiled for tests/test_register_budget.py
tests/hostcheck/libpfldscheck.so: tests/hostcheck/pfldscheck.hip $(CSRC)/prefilter_lds.hpp $(CSRC)/prefilter_record.hpp $(CSRC)/prefilter_math.hpp $(CSRC)/device_math.hpp
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the packed scan's decode of a survivor's bit position without its table (prefilter_math.hpp: pf_pack_code_closed), a host PROGRAM
# that prints it next to the table's entries and walks survivor masks through both, and says which epilogue the launcher picks for a
# launch's size (prefilter_lds.hpp: pf_sums_counts_at), for tests/test_pf_decode.py
tests/hostcheck/pfdecodecheck: tests/hostcheck/pfdecodecheck.hip $(CSRC)/prefilter_math.hpp $(CSRC)/prefilter_lds.hpp $(CSRC)/prefilter_record.hpp $(CSRC)/device_math.hpp
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -Wno-pass-failed -o $@ $<

# the per-tile rule's operands built once per hypothesis (prefilter_record.hpp: pf_tile_operands_full, the paired passes) against the
# per-half build of the single passes, host-compiled for tests/test_pf_pair_host.py
tests/hostcheck/libpfpaircheck.so: tests/hostcheck/pfpaircheck.hip $(CSRC)/prefilter_record.hpp $(CSRC)/prefilter_math.hpp $(CSRC)/device_math.hpp
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the row a ring entry of the paired passes decides on (prefilter_math.hpp: pf_ring_row and the tag's scan bit), host-compiled for
# tests/test_pf_ring_carry_host.py
tests/hostcheck/libpfringcheck.so: tests/hostcheck/pfringcheck.hip $(CSRC)/prefilter_math.hpp $(CSRC)/device_math.hpp
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the gate of sfm_match_guided and the arithmetic of sfm_pair_fundamental (match_guided_math.hpp) with a serial driver of the whole
# call (its own top-2 rule, score chain and emit formulae), for tests/test_match_guided_host.py and the field-by-field comparison
# of tests/test_gpu_match_guided.py; the no-scratch pin of match_guided.hip reads $(BUILD)/match_guided.usage.txt, which the object
# rule above writes
tests/hostcheck/libmatchguidedcheck.so: tests/hostcheck/matchguidedcheck.hip $(CSRC)/match_guided_math.hpp $(CSRC)/device_math.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -ffp-contract=off -mfma -fPIC -shared -Wno-pass-failed -o $@ $<

# the job layout and matcher-launch grouping of a batched sfm_process_pairs call (pairs_batch.hpp), host-compiled for
# tests/test_pairs_plan_host.py
tests/hostcheck/libpairsplancheck.so: tests/hostcheck/pairsplancheck.hip $(CSRC)/pairs_batch.hpp $(CSRC)/common.hpp $(CSRC)/pair_state.hpp include/sfm_amd.h
	$(HIPCC) -x hip --cuda-host-only -O2 -fPIC -shared -Wall -Wno-pass-failed -o $@ $<

# the pair's stage bookkeeping (pair_state.hpp), built by the plain host compiler for tests/test_pair_state_host.py
tests/hostcheck/libpairstatecheck.so: tests/hostcheck/pairstatecheck.cpp $(CSRC)/pair_state.hpp
	g++ -O2 -std=c++17 -Wall -fPIC -shared -o $@ $<

# the buffer-range rules of the batched calls (buffer_ranges.hpp) and the job order of their launches (job_order.hpp), built by
# the plain host compiler for tests/test_buffer_ranges_host.py
tests/hostcheck/libbufferrangescheck.so: tests/hostcheck/bufferrangescheck.cpp $(CSRC)/buffer_ranges.hpp $(CSRC)/job_order.hpp
	g++ -O2 -std=c++17 -Wall -fPIC -shared -o $@ $<

# the launch planner of sfm_match_guided_pairs (match_guided_plan.hpp) and the buffer rule across jobs that may overlap themselves
# (buffer_ranges.hpp), built by the plain host compiler for tests/test_match_guided_pairs_host.py; the no-scratch pin of
# match_guided_pairs.hip reads $(BUILD)/match_guided_pairs.usage.txt, which the object rule above writes.  -Bsymbolic-functions: the
# probe replaces operator new to record its own largest request, and its calls must bind to that replacement
tests/hostcheck/libmatchguidedplancheck.so: tests/hostcheck/matchguidedplancheck.cpp $(CSRC)/match_guided_plan.hpp $(CSRC)/buffer_ranges.hpp include/sfm_amd.h
	g++ -O2 -std=c++17 -Wall -fPIC -shared -Wl,-Bsymbolic-functions -o $@ $<

clean:
	rm -rf $(BUILD) $(LIB) $(LIB_AB) $(DEMO) $(HDEMO) $(SDEMO) $(MAINAPP) $(RPDEMO) $(RVDEMO) $(APDEMO) $(FCDEMO) $(GMDEMO) $(GPDEMO) $(IOTEST) $(GEOMTEST) tests/hostcheck/libhostcheck.so tests/hostcheck/librefinecheck.so tests/hostcheck/libregistercheck.so tests/hostcheck/libviewpointscheck.so tests/hostcheck/libadjustcheck.so tests/hostcheck/libaligncheck.so tests/hostcheck/libfusecheck.so tests/hostcheck/libchainadjustcheck.so tests/hostcheck/libringcheck.so tests/hostcheck/libfuseringcheck.so tests/hostcheck/libringadjustcheck.so tests/hostcheck/libintersectcheck.so tests/hostcheck/libpairstatecheck.so tests/hostcheck/libbufferrangescheck.so tests/hostcheck/libpfldscheck.so tests/hostcheck/libpairsplancheck.so tests/hostcheck/pfdecodecheck tests/hostcheck/libpfpaircheck.so tests/hostcheck/libpfringcheck.so tests/hostcheck/libmatchguidedcheck.so tests/hostcheck/libmatchguidedplancheck.so tests/fake_ccl/libsfm_amd_fakeccl.so
	$(MAKE) -C oracle clean

.PHONY: all ab oracle hostcheck fakeccl clean
