# Builds the product library roki-fd_amd/librkfd_amd.so (host C + HIP for gfx950),
# the CPU oracle (test infrastructure) and the lane-emulator harness (test infrastructure).
HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
CXX     ?= g++
ARCH    ?= gfx950
PKG      = roki-fd_amd
CSRC     = $(PKG)/csrc
BUILD    = $(PKG)/build
INC      = -Iinclude -I$(CSRC) -I$(CSRC)/host -I$(BUILD)
CFLAGS   = -O2 -Wall -fPIC $(INC)
# machine LICM off: hoisted literals / addresses held across the step loop cost ~35 VGPRs and the third wave per SIMD
ROCM_LIBDIR ?= $(abspath $(dir $(realpath $(HIPCC)))/../lib)
HIPFLAGS = --offload-arch=$(ARCH) -O3 -fPIC $(INC) -Wno-unused-value -mllvm -disable-machine-licm -DRKFD_ROCM_LIBDIR='"$(ROCM_LIBDIR)"'

HOST_OBJS = $(BUILD)/rkfd_ztk.o $(BUILD)/rkfd_world.o $(BUILD)/rkfd_sim.o $(BUILD)/rkfd_devmodel.o
LIB = $(PKG)/librkfd_amd.so

all: $(LIB) oracle emu spec

$(BUILD):
	mkdir -p $(BUILD)

$(BUILD)/%.o: $(CSRC)/host/%.c include/*.h $(CSRC)/host/*.h | $(BUILD)
	$(CC) $(CFLAGS) -c $< -o $@

$(BUILD)/rkfd_devmodel.o: $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h | $(BUILD)
	$(CXX) -std=c++17 $(CFLAGS) -c $< -o $@

# the compiler's per-kernel resource report is kept beside the object: tests/test_build_resources.py checks that no
# kernel spills to scratch and that all of them fit three waves per SIMD (168 VGPRs)
# the device sources as string literals inside the library: rkfdBatchSpecialize (hipRTC) needs no source files at run time
DEVSRC = include/rkfd_model.h $(CSRC)/rkfd_devmodel.h $(CSRC)/rkfd_device.h $(sort $(wildcard $(CSRC)/device/*.h))
$(BUILD)/rkfd_device_src.inc: $(DEVSRC) tools/embed_sources.py | $(BUILD)
	python3 tools/embed_sources.py $@ $(DEVSRC)

$(BUILD)/rkfd_capi.o: $(CSRC)/rkfd_capi.hip $(CSRC)/rkfd_capi_node.inc $(BUILD)/rkfd_device_src.inc $(CSRC)/*.h $(CSRC)/device/*.h $(CSRC)/readout/rkfd_links_host.h $(CSRC)/readout/rkfd_jac_host.h $(CSRC)/readout/rkfd_dyn_host.h $(CSRC)/readout/rkfd_cf_host.h $(CSRC)/reset/rkfd_reset_host.h include/*.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/rkfd_capi.remarks || ( cat $(BUILD)/rkfd_capi.remarks; exit 1 )
	@grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|VGPRs Spill|SGPRs Spill" $(BUILD)/rkfd_capi.remarks | sed 's/.*remark: *//; s/ \[-Rpass.*//' > $(PKG)/kernel_resources.txt
	@grep -vE "remark:|^ +[0-9]+ \||^ +\||\^" $(BUILD)/rkfd_capi.remarks || true

# the same step kernels built for batches that carry per-instance physical parameters (RKFD_PARAMS = 1): their own report
$(BUILD)/rkfd_capi_par.o: $(CSRC)/rkfd_capi_par.hip $(CSRC)/*.h $(CSRC)/device/*.h include/*.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/rkfd_capi_par.remarks || ( cat $(BUILD)/rkfd_capi_par.remarks; exit 1 )
	@grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|VGPRs Spill|SGPRs Spill" $(BUILD)/rkfd_capi_par.remarks | sed 's/.*remark: *//; s/ \[-Rpass.*//' > $(PKG)/kernel_resources_par.txt

# the task-space read-out (rkfdBatchUpdateLinks): a kernel and a translation unit of its own, outside the step kernels' sources: its own report
$(BUILD)/rkfd_capi_links.o: $(CSRC)/rkfd_capi_links.hip $(CSRC)/readout/*.h $(CSRC)/*.h $(CSRC)/device/rkfd_dev_base.h include/*.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/rkfd_capi_links.remarks || ( cat $(BUILD)/rkfd_capi_links.remarks; exit 1 )
	@grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|VGPRs Spill|SGPRs Spill" $(BUILD)/rkfd_capi_links.remarks | sed 's/.*remark: *//; s/ \[-Rpass.*//' > $(PKG)/kernel_resources_links.txt

# the task-space Jacobians (rkfdBatchUpdateJacobians): a kernel and a translation unit of its own, like the read-out: its own report
$(BUILD)/rkfd_capi_jac.o: $(CSRC)/rkfd_capi_jac.hip $(CSRC)/readout/rkfd_jac.h $(CSRC)/readout/rkfd_jac_host.h $(CSRC)/*.h $(CSRC)/device/rkfd_dev_base.h include/*.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/rkfd_capi_jac.remarks || ( cat $(BUILD)/rkfd_capi_jac.remarks; exit 1 )
	@grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|VGPRs Spill|SGPRs Spill" $(BUILD)/rkfd_capi_jac.remarks | sed 's/.*remark: *//; s/ \[-Rpass.*//' > $(PKG)/kernel_resources_jac.txt

# the joint-space dynamics (rkfdBatchUpdateDynamics): a kernel and a translation unit of its own, like the Jacobians: its own report
$(BUILD)/rkfd_capi_dyn.o: $(CSRC)/rkfd_capi_dyn.hip $(CSRC)/readout/rkfd_dyn.h $(CSRC)/readout/rkfd_dyn_host.h $(CSRC)/*.h $(CSRC)/device/rkfd_dev_base.h include/*.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/rkfd_capi_dyn.remarks || ( cat $(BUILD)/rkfd_capi_dyn.remarks; exit 1 )
	@grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|VGPRs Spill|SGPRs Spill" $(BUILD)/rkfd_capi_dyn.remarks | sed 's/.*remark: *//; s/ \[-Rpass.*//' > $(PKG)/kernel_resources_dyn.txt

# the contact read-out (rkfdBatchUpdateContactForces): a kernel and a translation unit of its own, like the dynamics: its own report
$(BUILD)/rkfd_capi_cf.o: $(CSRC)/rkfd_capi_cf.hip $(CSRC)/readout/rkfd_cf.h $(CSRC)/readout/rkfd_cf_host.h $(CSRC)/readout/rkfd_jac.h $(CSRC)/*.h $(CSRC)/device/rkfd_dev_base.h include/*.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/rkfd_capi_cf.remarks || ( cat $(BUILD)/rkfd_capi_cf.remarks; exit 1 )
	@grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|VGPRs Spill|SGPRs Spill" $(BUILD)/rkfd_capi_cf.remarks | sed 's/.*remark: *//; s/ \[-Rpass.*//' > $(PKG)/kernel_resources_cf.txt

# the per-instance reset (rkfdBatchReset) and its bank of start states: a kernel and a translation unit of its own, like the read-out: its own report
$(BUILD)/rkfd_capi_reset.o: $(CSRC)/rkfd_capi_reset.hip $(CSRC)/reset/*.h $(CSRC)/rkfd_devmodel.h include/*.h | $(BUILD)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c $< -o $@ 2> $(BUILD)/rkfd_capi_reset.remarks || ( cat $(BUILD)/rkfd_capi_reset.remarks; exit 1 )
	@grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|VGPRs Spill|SGPRs Spill" $(BUILD)/rkfd_capi_reset.remarks | sed 's/.*remark: *//; s/ \[-Rpass.*//' > $(PKG)/kernel_resources_reset.txt

$(LIB): $(HOST_OBJS) $(BUILD)/rkfd_capi.o $(BUILD)/rkfd_capi_par.o $(BUILD)/rkfd_capi_links.o $(BUILD)/rkfd_capi_reset.o $(BUILD)/rkfd_capi_jac.o $(BUILD)/rkfd_capi_dyn.o $(BUILD)/rkfd_capi_cf.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lm -ldl -lpthread

oracle:
	$(MAKE) -C oracle

# ahead-of-time specialised kernels: the code objects of the worlds of BASELINE.json's configurations, made now (hipRTC works
# without a GPU) and only LOADED at run time (rkfd_capi.hip: the store under $(PKG)/spec)
spec: $(LIB)
	python3 tools/make_spec.py

emu: tests/emu/librkfd_emu.so tests/emu/librkfd_emu_w2.so tests/emu/librkfd_emu_ctrl.so tests/emu/librkfd_emu_ctrl_w2.so \
     tests/emu/librkfd_emu_par.so tests/emu/librkfd_emu_par_w2.so tests/emu/librkfd_emu_links.so tests/emu/librkfd_emu_reset.so \
     tests/emu/librkfd_emu_jac.so tests/emu/librkfd_emu_dyn.so tests/emu/librkfd_emu_cf.so tests/emu/librkfd_emu_prim.so

tests/emu/librkfd_emu.so: tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread $(INC) -o $@ tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_devmodel.cpp

# the same harness with two instances per wavefront (RKFD_W = 2, rkfd_devmodel.h)
tests/emu/librkfd_emu_w2.so: tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread -DRKFD_W=2 $(INC) -o $@ tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_devmodel.cpp

# the harness with control schedules (rkfdBatchUpdateControlled's launches), one and two instances per wavefront
tests/emu/librkfd_emu_ctrl.so: tests/emu/rkfd_emu_ctrl.cpp tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread $(INC) -o $@ tests/emu/rkfd_emu_ctrl.cpp $(CSRC)/rkfd_devmodel.cpp

tests/emu/librkfd_emu_ctrl_w2.so: tests/emu/rkfd_emu_ctrl.cpp tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread -DRKFD_W=2 $(INC) -o $@ tests/emu/rkfd_emu_ctrl.cpp $(CSRC)/rkfd_devmodel.cpp

# the harness with a table of per-instance physical parameters (rkfdBatchSetParam's launches), one and two instances per wavefront
tests/emu/librkfd_emu_par.so: tests/emu/rkfd_emu_par.cpp tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread -DRKFD_PARAMS=1 $(INC) -o $@ tests/emu/rkfd_emu_par.cpp $(CSRC)/rkfd_devmodel.cpp

tests/emu/librkfd_emu_par_w2.so: tests/emu/rkfd_emu_par.cpp tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread -DRKFD_W=2 -DRKFD_PARAMS=1 $(INC) -o $@ tests/emu/rkfd_emu_par.cpp $(CSRC)/rkfd_devmodel.cpp

# the harness of the task-space read-out (readout/rkfd_links.h, the device code of rkfdBatchUpdateLinks)
tests/emu/librkfd_emu_links.so: tests/emu/rkfd_emu_links.cpp tests/emu/rkfd_emu.cpp $(CSRC)/readout/*.h $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread $(INC) -o $@ tests/emu/rkfd_emu_links.cpp $(CSRC)/rkfd_devmodel.cpp

# the harness of the task-space Jacobians (readout/rkfd_jac.h, the device code of rkfdBatchUpdateJacobians)
tests/emu/librkfd_emu_jac.so: tests/emu/rkfd_emu_jac.cpp tests/emu/rkfd_emu.cpp $(CSRC)/readout/*.h $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread $(INC) -o $@ tests/emu/rkfd_emu_jac.cpp $(CSRC)/rkfd_devmodel.cpp

# the harness of the joint-space dynamics (readout/rkfd_dyn.h, the device code of rkfdBatchUpdateDynamics)
tests/emu/librkfd_emu_dyn.so: tests/emu/rkfd_emu_dyn.cpp tests/emu/rkfd_emu.cpp $(CSRC)/readout/*.h $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread $(INC) -o $@ tests/emu/rkfd_emu_dyn.cpp $(CSRC)/rkfd_devmodel.cpp

# the harness of the contact read-out (readout/rkfd_cf.h, the device code of rkfdBatchUpdateContactForces)
tests/emu/librkfd_emu_cf.so: tests/emu/rkfd_emu_cf.cpp tests/emu/rkfd_emu.cpp $(CSRC)/readout/*.h $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread $(INC) -o $@ tests/emu/rkfd_emu_cf.cpp $(CSRC)/rkfd_devmodel.cpp

# the rotation primitives of device/rkfd_dev_base.h (d_sincos, d_atan2_ypos, d_from_aa, d_to_aa) as plain loops
tests/emu/librkfd_emu_prim.so: tests/emu/rkfd_emu_prim.cpp tests/emu/rkfd_emu.cpp $(CSRC)/rkfd_device.h $(CSRC)/rkfd_devmodel.cpp $(CSRC)/*.h $(CSRC)/device/*.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread $(INC) -o $@ tests/emu/rkfd_emu_prim.cpp $(CSRC)/rkfd_devmodel.cpp

# the harness of the per-instance reset (reset/rkfd_reset.h, the device code of rkfdBatchReset)
tests/emu/librkfd_emu_reset.so: tests/emu/rkfd_emu_reset.cpp $(CSRC)/reset/rkfd_reset.h $(CSRC)/rkfd_devmodel.h include/*.h
	$(CXX) -std=c++20 -O2 -Wall -Wno-unknown-pragmas -fPIC -shared -pthread $(INC) -o $@ tests/emu/rkfd_emu_reset.cpp

clean:
	rm -rf $(BUILD) $(LIB) $(PKG)/spec $(PKG)/kernel_resources_links.txt tests/emu/librkfd_emu_links.so $(PKG)/kernel_resources_reset.txt tests/emu/librkfd_emu_reset.so $(PKG)/kernel_resources_jac.txt tests/emu/librkfd_emu_jac.so $(PKG)/kernel_resources_dyn.txt tests/emu/librkfd_emu_dyn.so $(PKG)/kernel_resources_cf.txt tests/emu/librkfd_emu_cf.so tests/emu/librkfd_emu_prim.so tests/emu/librkfd_emu.so tests/emu/librkfd_emu_w2.so tests/emu/librkfd_emu_ctrl.so tests/emu/librkfd_emu_ctrl_w2.so tests/emu/librkfd_emu_par.so tests/emu/librkfd_emu_par_w2.so
	$(MAKE) -C oracle clean

.PHONY: all oracle emu spec clean
