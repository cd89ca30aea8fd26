# Builds the HIP extension in-tree (the .so travels to the GPU box with the repo snapshot).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := montgomery_amd/csrc
LIB := montgomery_amd/libmsm_hip.so
HIPFLAGS := -O3 -pthread -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall -Wno-unused-function -Wno-unused-variable \
            -Iinclude -I$(CSRC)
BUILD := build
CURVES := CvBls377 CvBls381 CvPallas CvBn254 CvGrumpkin CvVesta
CURVE_OBJS := $(CURVES:%=$(BUILD)/kernels_%.o)
HOST_TUS := msm_plan msm_sort msm_tree msm_reduce msm_upload msm_pipeline msm_batch msm_tables msm_abi msm_test_abi msm_gen msm_ingest msm_narrow msm_indexed msm_lincomb msm_points_mul msm_points_ntt msm_scalars msm_ntt msm_scan msm_mle msm_spmv sort_kernels te_kernels narrow_kernels
HOST_OBJS := $(HOST_TUS:%=$(BUILD)/%.o)
KHDRS := $(CSRC)/msm_kernels.h $(CSRC)/batch_add.h $(CSRC)/msm_gen_kernels.h $(CSRC)/kernel_inst.h $(CSRC)/field.h $(CSRC)/packed.h $(CSRC)/curve.h \
         $(CSRC)/glv.h $(CSRC)/constants_gen.h

# the curve-templated kernels compile once per curve, in parallel with the host pipeline
all:
	$(MAKE) -j8 $(LIB)

$(CSRC)/constants_gen.h: $(CSRC)/gen_constants.py
	python3 $(CSRC)/gen_constants.py

$(BUILD)/kernels_%.o: $(CSRC)/kernels_curve.hip $(KHDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) -DMSM_CURVE_TU=$* -c $(CSRC)/kernels_curve.hip -o $@

# the host pipeline is one translation unit per concern (msm_internal.h lists them); the curve-independent kernels have two of their own
HHDRS := $(KHDRS) $(CSRC)/points_ingest.h $(CSRC)/points_lincomb.h $(CSRC)/points_mul.h $(CSRC)/points_ntt.h $(CSRC)/scalar_vec.h $(CSRC)/scalar_ntt.h $(CSRC)/scalar_scan.h $(CSRC)/scalar_mle.h $(CSRC)/scalar_spmv.h $(CSRC)/scalar_host.h $(CSRC)/msm_internal.h $(CSRC)/operator_checks.h $(CSRC)/sort_kernels.h $(CSRC)/tree_kernels.h $(CSRC)/te_kernels.h $(CSRC)/narrow_kernels.h $(CSRC)/host_field.h include/msm_hip.h
# msm_points_mul: with the loop-invariant code motion of the machine passes, every constant of the row loop's body (the GLV
# vectors, q, p, beta) is kept in a scalar register across the whole loop and up to 37 of them go to vector lanes and back
TUFLAGS_msm_points_mul := -mllvm -disable-machine-licm
# msm_points_ntt: its stage kernel is that row loop with a butterfly behind the walk
TUFLAGS_msm_points_ntt := -mllvm -disable-machine-licm
$(BUILD)/%.o: $(CSRC)/%.hip $(HHDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) $(HIPFLAGS) $(TUFLAGS_$*) -c $< -o $@

$(LIB): $(HOST_OBJS) $(CURVE_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -pthread $(HOST_OBJS) $(CURVE_OBJS) -o $(LIB)

clean:
	rm -rf $(LIB) $(BUILD)

.PHONY: all clean ab ab_pmul

# CPU build of the field / GLV templates for tests/test_host_field.py (no GPU needed)
HOSTTEST := tests/csrc/libfield_host.so
HOSTTEST_CYCLES := tests/csrc/libfield_host_cycles.so
HOSTTEST_LINCOMB := tests/csrc/liblincomb_host.so
HOSTTEST_SCALARS := tests/csrc/libscalars_host.so
HOSTTEST_SCHEDULE := tests/csrc/libschedule_host.so
HOSTTEST_NTT := tests/csrc/libntt_host.so
HOSTTEST_SCANS := tests/csrc/libscans_host.so
HOSTTEST_PMUL := tests/csrc/libpoints_mul_host.so
HOSTTEST_PNTT := tests/csrc/libpoints_ntt_host.so
HOSTTEST_SCALAR_HOST := tests/csrc/libscalar_host_host.so
HOSTTEST_MLE := tests/csrc/libmle_host.so
HOSTTEST_SPMV := tests/csrc/libspmv_host.so
# (every shim whose source the tests tree holds: a tests tree from before the schedule shim still builds the others)
hosttest: $(HOSTTEST) $(HOSTTEST_CYCLES) $(HOSTTEST_LINCOMB) $(HOSTTEST_SCALARS) $(if $(wildcard tests/csrc/schedule_host.hip),$(HOSTTEST_SCHEDULE)) \
          $(if $(wildcard tests/csrc/ntt_host.hip),$(HOSTTEST_NTT)) $(if $(wildcard tests/csrc/scans_host.hip),$(HOSTTEST_SCANS)) \
          $(if $(wildcard tests/csrc/points_mul_host.hip),$(HOSTTEST_PMUL)) $(if $(wildcard tests/csrc/scalar_host_host.hip),$(HOSTTEST_SCALAR_HOST)) \
          $(if $(wildcard tests/csrc/mle_host.hip),$(HOSTTEST_MLE)) $(if $(wildcard tests/csrc/spmv_host.hip),$(HOSTTEST_SPMV)) \
          $(if $(wildcard tests/csrc/points_ntt_host.hip),$(HOSTTEST_PNTT))
# scalar_host.h on all seven scalar fields and the range and row rules of operator_checks.h, whose refusals go through the fail() of
# msm_plan.hip over a bare context: tests/test_scalar_host.py
$(HOSTTEST_SCALAR_HOST): tests/csrc/scalar_host_host.hip $(CSRC)/msm_plan.hip $(HHDRS)
	$(HIPCC) -O2 -pthread -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Wno-unused-value -Iinclude -I$(CSRC) tests/csrc/scalar_host_host.hip $(CSRC)/msm_plan.hip -o $(HOSTTEST_SCALAR_HOST)
# the window-group schedule of msm_plan.hip (group_schedule: no HIP call) over a bare context: tests/test_group_schedule.py
$(HOSTTEST_SCHEDULE): tests/csrc/schedule_host.hip $(CSRC)/msm_plan.hip $(HHDRS)
	$(HIPCC) -O2 -pthread -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Wno-unused-value -Iinclude -I$(CSRC) tests/csrc/schedule_host.hip $(CSRC)/msm_plan.hip -o $(HOSTTEST_SCHEDULE)
# the plan, the index functions and the lane bodies of scalar_ntt.h, run lane by lane on the host: tests/test_ntt_host.py
$(HOSTTEST_NTT): tests/csrc/ntt_host.hip $(CSRC)/field.h $(CSRC)/constants_gen.h $(CSRC)/scalar_vec.h $(CSRC)/scalar_host.h $(CSRC)/scalar_ntt.h include/msm_hip.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Iinclude -I$(CSRC) tests/csrc/ntt_host.hip -o $(HOSTTEST_NTT)
# the plan, the combine operators and the inverse lane body of scalar_scan.h on the host: tests/test_scans_host.py
$(HOSTTEST_SCANS): tests/csrc/scans_host.hip $(CSRC)/field.h $(CSRC)/constants_gen.h $(CSRC)/scalar_vec.h $(CSRC)/scalar_host.h $(CSRC)/scalar_scan.h include/msm_hip.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Iinclude -I$(CSRC) tests/csrc/scans_host.hip -o $(HOSTTEST_SCANS)
# the index maps, the lane bodies and the half-table split of scalar_mle.h on the host: tests/test_mle_host.py
$(HOSTTEST_MLE): tests/csrc/mle_host.hip $(CSRC)/field.h $(CSRC)/constants_gen.h $(CSRC)/scalar_vec.h $(CSRC)/scalar_host.h $(CSRC)/scalar_mle.h include/msm_hip.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Iinclude -I$(CSRC) tests/csrc/mle_host.hip -o $(HOSTTEST_MLE)
# the CSR rule, the plan, the transposition and the lane bodies of scalar_spmv.h on the host: tests/test_spmv_host.py
$(HOSTTEST_SPMV): tests/csrc/spmv_host.hip $(CSRC)/field.h $(CSRC)/constants_gen.h $(CSRC)/scalar_vec.h $(CSRC)/scalar_host.h $(CSRC)/scalar_mle.h $(CSRC)/scalar_spmv.h include/msm_hip.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Iinclude -I$(CSRC) tests/csrc/spmv_host.hip -o $(HOSTTEST_SPMV)
# the lane bodies of scalar_vec.h on the scalar fields of all seven curves: tests/test_scalars_host.py
$(HOSTTEST_SCALARS): tests/csrc/scalars_host.hip $(CSRC)/field.h $(CSRC)/constants_gen.h $(CSRC)/scalar_vec.h $(CSRC)/scalar_host.h include/msm_hip.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Iinclude -I$(CSRC) tests/csrc/scalars_host.hip -o $(HOSTTEST_SCALARS)
# the recoder and the lane bodies of points_lincomb.h on all seven curves: tests/test_points_lincomb_host.py
$(HOSTTEST_LINCOMB): tests/csrc/lincomb_host.hip $(KHDRS) $(CSRC)/points_ingest.h $(CSRC)/points_lincomb.h $(CSRC)/te_kernels.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Wno-unused-value -Iinclude -I$(CSRC) tests/csrc/lincomb_host.hip -o $(HOSTTEST_LINCOMB)
# the recoding and the lane bodies of points_mul.h on all seven curves, at every candidate window: tests/test_points_mul_host.py
$(HOSTTEST_PMUL): tests/csrc/points_mul_host.hip $(KHDRS) $(CSRC)/points_mul.h $(CSRC)/te_kernels.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Wno-unused-value -Iinclude -I$(CSRC) tests/csrc/points_mul_host.hip -o $(HOSTTEST_PMUL)
# the index maps and the butterfly lane of points_ntt.h on the host: tests/test_points_ntt_host.py
$(HOSTTEST_PNTT): tests/csrc/points_ntt_host.hip $(KHDRS) $(CSRC)/points_mul.h $(CSRC)/points_ntt.h $(CSRC)/te_kernels.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Wno-unused-value -Iinclude -I$(CSRC) tests/csrc/points_ntt_host.hip -o $(HOSTTEST_PNTT)
# the cycle curves (BN254 G1, Grumpkin, Vesta), with the square root of points_ingest.h: tests/test_cycle_curves.py
$(HOSTTEST_CYCLES): tests/csrc/field_host_cycles.hip $(KHDRS) $(CSRC)/points_ingest.h $(CSRC)/te_kernels.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -Wno-unused-value -Iinclude -I$(CSRC) tests/csrc/field_host_cycles.hip -o $(HOSTTEST_CYCLES)
$(HOSTTEST): tests/csrc/field_host.hip $(CSRC)/field.h $(CSRC)/glv.h $(CSRC)/constants_gen.h
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -I$(CSRC) tests/csrc/field_host.hip -o $(HOSTTEST)

# Node N-API shim (the image's node 12 exposes N-API 8 through /usr/include/node)
NAPI := montgomery_amd/msm_hip.node
napi: $(NAPI)
$(NAPI): napi/msm_addon.cc include/msm_hip.h $(LIB)
	g++ -O2 -std=c++14 -fPIC -shared -Iinclude -I/usr/include/node napi/msm_addon.cc -o $(NAPI) \
	    -Lmontgomery_amd -lmsm_hip -Wl,-rpath,'$$ORIGIN'

# plain-C host of the C ABI (no Python): examples/msm_demo [log2_n] [curve]
demo: examples/msm_demo
examples/msm_demo: examples/msm_demo.c include/msm_hip.h $(LIB)
	gcc -O2 -Wall -Iinclude examples/msm_demo.c -Lmontgomery_amd -lmsm_hip -Wl,-rpath,'$$ORIGIN/../montgomery_amd' -o examples/msm_demo

# A/B experiment builds of the extension: make ab NAME=w2 EXTRA="-DMSM_BA_WAVES=2"  ->  ab_builds/libmsm_w2.so
# (timed against each other by tools/ab_time.py through MSM_HIP_LIB; ab_builds/ is not tracked)
ab:
	@mkdir -p ab_builds/$(NAME)
	for c in $(CURVES); do $(HIPCC) $(HIPFLAGS) $(EXTRA) -DMSM_CURVE_TU=$$c -c $(CSRC)/kernels_curve.hip -o ab_builds/$(NAME)/kernels_$$c.o & done; \
	$(foreach t,$(HOST_TUS),$(HIPCC) $(HIPFLAGS) $(TUFLAGS_$(t)) $(EXTRA) -c $(CSRC)/$(t).hip -o ab_builds/$(NAME)/$(t).o & ) wait
	$(HIPCC) --offload-arch=$(ARCH) -shared -pthread ab_builds/$(NAME)/*.o -o ab_builds/libmsm_$(NAME).so
	rm -rf ab_builds/$(NAME)

# the same for the candidates of msm_points_mul, which differ in one translation unit: make ab_pmul NAME=w5 EXTRA="-DMSM_PMUL_W=5"
# links ab_builds/libmsm_pmul_w5.so from that unit and the in-tree objects (tools/bench_points_mul.py --libs times them)
ab_pmul: $(LIB)
	@mkdir -p ab_builds
	$(HIPCC) $(HIPFLAGS) $(TUFLAGS_msm_points_mul) $(EXTRA) -c $(CSRC)/msm_points_mul.hip -o ab_builds/pmul_$(NAME).o
	$(HIPCC) --offload-arch=$(ARCH) -shared -pthread $(filter-out $(BUILD)/msm_points_mul.o,$(HOST_OBJS)) ab_builds/pmul_$(NAME).o $(CURVE_OBJS) -o ab_builds/libmsm_pmul_$(NAME).so
	rm -f ab_builds/pmul_$(NAME).o

# micro-benchmarks quoted in DESIGN.md (run on the GPU box; outputs are committed under profiles/)
UBENCH := ubench_int2 ubench_inv ubench_mul2 ubench_mad3 ubench_gather ubench_carry
ubench:
	for u in $(UBENCH); do $(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -Iinclude -I$(CSRC) tools/$$u.hip -o tools/$$u 2>&1 | grep -E "error" ; done; true
