# Top-level build. `make` produces the in-tree HIP library and the
# reference-shaped ./Application (so the reference's grader flow
# `make && ./Application testcases/X.conf` runs against this build).
#   distributed-membership_amd/lib/libgm.so   hand-written HIP (gfx950) + C ABI
#   ./Application                             host C++ driver (Application/Params/Log surface)
#   oracle/build/*                            CPU restatement (test infrastructure)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := distributed-membership_amd
CSRC := $(PKG)/csrc
HIPFLAGS := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Iinclude -I$(CSRC) -Wall -Wno-unused-result
LIB := $(PKG)/lib/libgm.so
KOBJS := $(PKG)/build/gm_faithful.o $(PKG)/build/gm_scaled.o $(PKG)/build/gm_band.o $(PKG)/build/gm_draw.o \
         $(PKG)/build/gm_partial.o $(PKG)/build/gm_partial_xchg.o $(PKG)/build/gm_detect.o \
         $(PKG)/build/gm_load.o $(PKG)/build/gm_census.o $(PKG)/build/gm_view_census.o $(PKG)/build/gm_read.o \
         $(PKG)/build/gm_load_views.o $(PKG)/build/gm_view_detect.o $(PKG)/build/gm_digest.o \
         $(PKG)/build/gm_view_reach.o $(PKG)/build/gm_view_reach_shard.o \
         $(PKG)/build/gm_host.o $(PKG)/build/gm_host_faithful.o $(PKG)/build/gm_host_batch.o $(PKG)/build/gm_host_scaled.o \
         $(PKG)/build/gm_host_shard.o $(PKG)/build/gm_host_partial.o $(PKG)/build/gm_host_events.o \
         $(PKG)/build/gm_host_read.o $(PKG)/build/gm_host_stage.o $(PKG)/build/gm_host_load.o \
         $(PKG)/build/gm_host_view_detect.o $(PKG)/build/gm_host_digest.o \
         $(PKG)/build/gm_host_view_reach.o
HDRS := include/gm_abi.h $(CSRC)/gm_device.h $(CSRC)/gm_faithful.h $(CSRC)/gm_scaled.h $(CSRC)/gm_partial.h \
        $(CSRC)/gm_partial_node.h $(CSRC)/gm_host.h $(CSRC)/gm_band.h $(CSRC)/gm_select.h $(CSRC)/gm_digest.h
# kernel files compiled as part of another unit (gm_band.hip, gm_draw.hip include them)
HDRS += $(CSRC)/gm_band_fast.hip $(CSRC)/gm_pick.hip
# the FAITHFUL kernel bodies, included as text by gm_faithful.hip
HDRS += $(CSRC)/gm_faithful_tick.h

all: $(LIB) Application oracle

$(PKG)/build/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(PKG)/build
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(KOBJS)
	@mkdir -p $(PKG)/lib
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(KOBJS) -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

Application: $(PKG)/app/Application.cpp $(PKG)/app/Log.cpp $(PKG)/app/Application.h $(PKG)/app/Log.h $(LIB)
	g++ -O2 -std=c++17 -Wall -Iinclude -I$(PKG)/app -o $@ $(PKG)/app/Application.cpp $(PKG)/app/Log.cpp \
	    -L$(PKG)/lib -lgm -Wl,-rpath,'$$ORIGIN/$(PKG)/lib'

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(PKG)/build $(PKG)/lib Application dbg.log stats.log msgcount.log
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
