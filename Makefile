# Build of libpptkrx.so (product) and the oracle (test infrastructure).
#   make            -> pptk_amd/libpptkrx.so + oracle/liboracle.so (+ oracle/_ref),
#                      tests/hooks/libpptkrx_hooks.so, harness/*.so
#   make tools      -> the probe libraries under tools/ (not built by default)
# gfx950 only; hipcc cross-compiles without a GPU.
HIPCC ?= /opt/rocm/bin/hipcc
CC ?= gcc
ARCH ?= gfx950
OBJDIR := build/obj
HIPFLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -Iinclude -I/opt/rocm/include
CFLAGS := -O2 -std=gnu11 -fPIC -Wall -Wextra -Iinclude

LIB := pptk_amd/libpptkrx.so
HIP_SRCS := pptk_amd/csrc/rx_kernel.hip pptk_amd/csrc/rx_bin.hip pptk_amd/csrc/rx_permit.hip \
            pptk_amd/csrc/rx_capi.hip pptk_amd/csrc/rx_comm.hip pptk_amd/csrc/rx_ring.hip \
            pptk_amd/csrc/tx_frag.hip pptk_amd/csrc/tx_tunnel.hip pptk_amd/csrc/tx_hdr.hip \
            pptk_amd/csrc/rx_flow.hip pptk_amd/csrc/rx_flowstat.hip pptk_amd/csrc/rx_flowlearn.hip \
            pptk_amd/csrc/rx_host.hip pptk_amd/csrc/ip_reass.hip pptk_amd/csrc/tx_dispatch.hip \
            pptk_amd/csrc/tx_gather.hip
C_SRCS := pptk_amd/csrc/host/ipcksum.c pptk_amd/csrc/host/hashseed.c pptk_amd/csrc/host/tcpopt.c \
          pptk_amd/csrc/host/iphash.c pptk_amd/csrc/host/timerlink.c pptk_amd/csrc/host/ipfrag.c \
          pptk_amd/csrc/host/tcpseq.c pptk_amd/csrc/host/tunnel.c pptk_amd/csrc/host/flowtab.c \
          pptk_amd/csrc/host/flowlearn.c pptk_amd/csrc/host/ipreass.c pptk_amd/csrc/host/dispatch.c \
          pptk_amd/csrc/host/gather.c
HDRS := $(wildcard include/*.h) pptk_amd/csrc/rx_internal.h pptk_amd/csrc/copy16.h \
        pptk_amd/csrc/frame_view.h pptk_amd/csrc/flowtab.h pptk_amd/csrc/host_plan.h \
        pptk_amd/csrc/dispatch_check.h pptk_amd/csrc/gather_check.h pptk_amd/csrc/block_scan.h \
        pptk_amd/csrc/scratch_carve.h pptk_amd/csrc/host/outer_ipv4.h
HIP_OBJS := $(patsubst pptk_amd/csrc/%.hip,$(OBJDIR)/%.o,$(HIP_SRCS))
C_OBJS := $(patsubst pptk_amd/csrc/host/%.c,$(OBJDIR)/host/%.o,$(C_SRCS))

all: $(LIB) oracle

$(OBJDIR)/%.o: pptk_amd/csrc/%.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJDIR)/host/%.o: pptk_amd/csrc/host/%.c $(HDRS)
	@mkdir -p $(dir $@)
	$(CC) $(CFLAGS) -c $< -o $@

$(LIB): $(HIP_OBJS) $(C_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -ldl

oracle:
	$(MAKE) -C oracle

# The test library: the product with its fault-injection knobs compiled in
# (-DPPTK_RX_TEST_HOOKS: a rate-limiter workgroup held past its barrier
# deadline, a stalled communicator warm-up).  Only the failure-path tests load
# it; the product library never reads those knobs.
HOOKS_LIB := tests/hooks/libpptkrx_hooks.so
HOOKS_SRCS := pptk_amd/csrc/rx_permit.hip pptk_amd/csrc/rx_comm.hip
HOOKS_OBJS := $(patsubst pptk_amd/csrc/%.hip,$(OBJDIR)/hooks/%.o,$(HOOKS_SRCS))

$(OBJDIR)/hooks/%.o: pptk_amd/csrc/%.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -DPPTK_RX_TEST_HOOKS -c $< -o $@

$(HOOKS_LIB): $(filter-out $(OBJDIR)/rx_permit.o $(OBJDIR)/rx_comm.o,$(HIP_OBJS)) $(HOOKS_OBJS) $(C_OBJS)
	@mkdir -p $(dir $@)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -ldl

hooks: $(HOOKS_LIB)
all: $(HOOKS_LIB)

# A/B builds of the product library with extra defines, e.g.
#   make abvariant NAME=flow4 DEFS=-DPPTK_FLOW_TEAM=4   (rx_flow.hip: four lanes per record)
#   make abvariant NAME=flowstat_direct DEFS=-DPPTK_FLOWSTAT_DIRECT=1   (rx_flowstat.hip: no LDS stage)
abvariant:
	$(MAKE) OBJDIR=build/ab_$(NAME)/obj LIB=build/ab_$(NAME)/libpptkrx.so \
	  HIPFLAGS="$(HIPFLAGS) $(DEFS)" build/ab_$(NAME)/libpptkrx.so

# the kernel files' assembly and resource tables (build/asm/<file>.resource.txt)
ASM_SRCS := rx_kernel tx_hdr rx_flowstat rx_flowlearn tx_dispatch ip_reass tx_frag tx_tunnel rx_flow tx_gather
asm: $(HIP_SRCS)
	@mkdir -p build/asm
	cd build/asm && for f in $(ASM_SRCS); do $(HIPCC) $(HIPFLAGS) -I../../include -c ../../pptk_amd/csrc/$$f.hip -save-temps -o $$f.o -Rpass-analysis=kernel-resource-usage 2> $$f.resource.txt; done; true

clean:
	rm -rf build $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean asm

# Measurement harness (bench.py and the GPU tests): synthetic frames generated
# in HBM and the trivial kernels that give the box's speed of light.
HARNESS_LIBS := harness/libpptksynth.so harness/libmembench.so harness/librwmix.so

harness/lib%.so: harness/%.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -fPIC -shared -std=c++17 -o $@ $<

harness/libpptksynth.so: harness/synth.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -fPIC -shared -std=c++17 -o $@ $<

all: $(HARNESS_LIBS)

# Probes (measured-and-kept evidence for DESIGN.md, not part of the product
# or of the default build): make tools
PROBE_LIBS := tools/libglds_probe.so tools/libteam_probe.so tools/libepoch_probe.so \
              tools/libstandin.so

tools/lib%.so: tools/%.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -fPIC -shared -std=c++17 -o $@ $<

tools: $(PROBE_LIBS)

.PHONY: tools
