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
KHDRS := $(CSRC)/msm_kernels.h $(CSRC)/batch_add.h $(CSRC)/mem_policy.h $(CSRC)/msm_gen_kernels.h $(CSRC)/kernel_inst.h $(CSRC)/field.h $(CSRC)/packed.h $(CSRC)/curve.h \
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

# CPU builds of the device headers for the host tests (no GPU needed): tests/csrc/<stem>.hip -> tests/csrc/lib<stem>.so, for every
# shim whose source the tests tree holds.  One recipe; a library differs from the next in the headers it is rebuilt for and, where
# said below, in a flag or a further source.
HT = $(1:%=tests/csrc/lib%.so)
hosttest: $(call HT,$(patsubst tests/csrc/%.hip,%,$(wildcard tests/csrc/*.hip)))
HT_INC := -Iinclude
tests/csrc/lib%.so: tests/csrc/%.hip
	$(strip $(HIPCC) -O2 $(HT_THREADS) -std=c++17 --offload-arch=$(ARCH) -fPIC -shared $(HT_WARN) $(HT_INC) -I$(CSRC) $< $(HT_MORE) -o $@)

SCALAR_HDRS := $(CSRC)/field.h $(CSRC)/constants_gen.h $(CSRC)/scalar_vec.h $(CSRC)/scalar_host.h include/msm_hip.h
POINT_HDRS := $(KHDRS) $(CSRC)/te_kernels.h
# the field / GLV templates alone, without the public header: tests/test_host_field.py
$(call HT,field_host): $(CSRC)/field.h $(CSRC)/glv.h $(CSRC)/constants_gen.h
$(call HT,field_host): HT_INC :=
# the cycle curves (BN254 G1, Grumpkin, Vesta), with the square root of points_ingest.h: tests/test_cycle_curves.py
$(call HT,field_host_cycles): $(POINT_HDRS) $(CSRC)/points_ingest.h
# the recoder and the lane bodies of points_lincomb.h on all seven curves: tests/test_points_lincomb_host.py
$(call HT,lincomb_host): $(POINT_HDRS) $(CSRC)/points_ingest.h $(CSRC)/points_lincomb.h
# the recoding and the lane bodies of points_mul.h on all seven curves, at every candidate window: tests/test_points_mul_host.py
$(call HT,points_mul_host): $(POINT_HDRS) $(CSRC)/points_mul.h
# the index maps and the butterfly lane of points_ntt.h on the host: tests/test_points_ntt_host.py
$(call HT,points_ntt_host): $(POINT_HDRS) $(CSRC)/points_mul.h $(CSRC)/points_ntt.h
# the lane bodies of scalar_vec.h on the scalar fields of all seven curves: tests/test_scalars_host.py
$(call HT,scalars_host): $(SCALAR_HDRS)
# the plan, the index functions and the lane bodies of scalar_ntt.h, run lane by lane on the host: tests/test_ntt_host.py
$(call HT,ntt_host): $(SCALAR_HDRS) $(CSRC)/scalar_ntt.h
# the plan, the combine operators and the inverse lane body of scalar_scan.h on the host: tests/test_scans_host.py
$(call HT,scans_host): $(SCALAR_HDRS) $(CSRC)/scalar_scan.h
# the index maps, the lane bodies and the half-table split of scalar_mle.h on the host: tests/test_mle_host.py
$(call HT,mle_host): $(SCALAR_HDRS) $(CSRC)/scalar_mle.h
# the CSR rule, the plan, the transposition and the lane bodies of scalar_spmv.h on the host: tests/test_spmv_host.py
$(call HT,spmv_host): $(SCALAR_HDRS) $(CSRC)/scalar_mle.h $(CSRC)/scalar_spmv.h
# over a bare context, with msm_plan.hip linked in: scalar_host.h on all seven scalar fields and the range and row rules of
# operator_checks.h, whose refusals go through its fail() (tests/test_scalar_host.py), and its window-group schedule
# (group_schedule: no HIP call; tests/test_group_schedule.py)
HT_BARE_CTX := $(call HT,scalar_host_host schedule_host)
$(HT_BARE_CTX): $(CSRC)/msm_plan.hip $(HHDRS)
$(HT_BARE_CTX): HT_THREADS := -pthread
$(HT_BARE_CTX): HT_MORE := $(CSRC)/msm_plan.hip
# the kernel headers hold expressions whose value a host build does not use
$(HT_BARE_CTX) $(call HT,field_host_cycles lincomb_host points_mul_host points_ntt_host): HT_WARN := -Wno-unused-value

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
