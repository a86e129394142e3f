# Builds the product library (build/libj40hip.so: host parser + HIP kernels for gfx950 + public API),
# the synthetic stream generator (build/jxlsynth) and the checkers under oracle/.
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
CXX ?= g++
ARCH ?= gfx950
CXXFLAGS = -std=c++17 -O2 -fPIC -Wall -Wextra -ffp-contract=off -fvisibility=hidden
# EVENT_RING=8 (or 4): k_hf_lanes' coefficient events leave through per-lane rings in LDS as aligned 32- (16-) byte stores
# (device/plan.h: J40_LANE_EV_FLUSH; default 0 = a 4-byte store per event). The CPU build of the device functions exists in both
# forms: libhostsim.so with the product's setting, libhostsim_ring8.so with the rings (tests/test_hostsim.py runs through both).
EVENT_RING ?= 0
CXXFLAGS += -DJ40_LANE_EV_FLUSH=$(EVENT_RING)
HIPFLAGS = --offload-arch=$(ARCH) -std=c++17 -O3 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fvisibility=hidden -Wall -DJ40_LANE_EV_FLUSH=$(EVENT_RING) $(EXTRA_HIPFLAGS)
SRC = j40_amd/csrc
HOST_OBJS = build/obj/plan_build.o build/obj/plan_front.o build/obj/entropy.o build/obj/modular.o build/obj/tables.o build/obj/frame.o build/obj/capi_host.o build/obj/api.o
DEV_OBJS = build/obj/kernels.o build/obj/modular_kernels.o build/obj/runtime.o build/obj/runtime_upload.o build/obj/runtime_lf.o build/obj/runtime_batch.o build/obj/runtime_lfp.o build/obj/runtime_debug.o build/obj/device_memory.o build/obj/pipeline.o build/obj/lf_tail_kernels.o build/obj/modular_coop.o build/obj/modular_quad.o build/obj/modular_split.o build/obj/lf_decode.o build/obj/plan_kernels.o build/obj/async.o build/obj/hostcopy.o build/obj/lf_preview.o build/obj/alpha_kernels.o build/obj/region_kernels.o build/obj/compose_kernels.o build/obj/runtime_seq.o build/obj/scale_kernels.o build/obj/ycbcr_kernels.o build/obj/orient_kernels.o build/obj/modular_xyb_kernels.o build/obj/colour_kernels.o build/obj/patch_kernels.o build/obj/noise_kernels.o build/obj/upsample_kernels.o build/obj/spline_kernels.o

.PHONY: all lib tools oracle hostsim clean print-objs
all: lib tools hostsim oracle
# the library's objects, for tools/build_variant.sh
print-objs:
	@echo $(HOST_OBJS) $(DEV_OBJS)
lib: build/libj40hip.so
tools: build/jxlsynth
oracle:
	$(MAKE) -C oracle all

build/obj/%.o: $(SRC)/%.cpp $(wildcard $(SRC)/*.hpp) $(wildcard $(SRC)/device/*.h) include/j40hip.h include/j40.h
	@mkdir -p build/obj
	$(CXX) $(CXXFLAGS) -c $< -o $@

build/obj/%.o: $(SRC)/device/%.hip $(wildcard $(SRC)/device/*.h) $(wildcard $(SRC)/device/*.hpp) $(wildcard $(SRC)/*.hpp) include/j40hip.h
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# lf_decode.hip: k_lf_rows steps two LfGroup sections per lane side by side; the two sections' instructions are independent and the
# scheduler is asked to interleave them rather than to keep register pressure low (a wavefront alone on its SIMD, 512 registers its own)
build/obj/lf_decode.o: EXTRA_HIPFLAGS += -mllvm -amdgpu-sched-strategy=max-ilp

build/libj40hip.so: $(HOST_OBJS) $(DEV_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^ -lpthread -lhsa-runtime64

# the stand-alone layout programs (below) belong to hostsim wherever tests/hostsim holds their source; the libraries do not need it
LAYOUTMAIN = $(if $(wildcard tests/hostsim/mod_layout_main.cpp),build/mod_layout_main build/mod_layout_main_san)
# (likewise the stand-alone programs of the reduced-size decode; defined here because a rule's prerequisites are expanded where it is read)
SCALEMAIN = $(if $(wildcard tests/hostsim/scale_main.cpp),build/scale_main build/scale_main_san)
HOSTSIM_HDR = $(wildcard $(SRC)/device/*.h) $(wildcard $(SRC)/*.hpp) $(wildcard tests/hostsim/*.hpp)
YCBCRMAIN = $(if $(wildcard tests/hostsim/ycbcr_main.cpp),build/ycbcr_main build/ycbcr_main_san)
ORIENTMAIN = $(if $(wildcard tests/hostsim/orient_main.cpp),build/orient_main build/orient_main_san)
WIDESIM = $(if $(wildcard tests/hostsim/wide_sim.cpp),build/libwidesim.so)
WIDEMAIN = $(if $(wildcard tests/hostsim/wide_main.cpp),build/wide_main build/wide_main_san)
MODXYBSIM = $(if $(wildcard tests/hostsim/modular_xyb_sim.cpp),build/libhostsim_modxyb.so)
MODXYBMAIN = $(if $(wildcard tests/hostsim/modular_xyb_main.cpp),build/modular_xyb_main build/modular_xyb_main_san)
COLOURSIM = $(if $(wildcard tests/hostsim/colour_sim.cpp),build/libhostsim_colour.so)
COLOURMAIN = $(if $(wildcard tests/hostsim/colour_main.cpp),build/colour_main build/colour_main_san)
PATCHSIM = $(if $(wildcard tests/hostsim/patch_sim.cpp),build/libhostsim_patches.so)
PATCHMAIN = $(if $(wildcard tests/hostsim/patch_main.cpp),build/patch_main build/patch_main_san)
NOISESIM = $(if $(wildcard tests/hostsim/noise_sim.cpp),build/libhostsim_noise.so)
NOISEMAIN = $(if $(wildcard tests/hostsim/noise_main.cpp),build/noise_main build/noise_main_san)
SPLINESIM = $(if $(wildcard tests/hostsim/spline_sim.cpp),build/libhostsim_splines.so)
SPLINEMAIN = $(if $(wildcard tests/hostsim/spline_main.cpp),build/spline_main build/spline_main_san)
UPSAMPLEMAIN = $(if $(wildcard tests/hostsim/upsample_main.cpp),build/upsample_main build/upsample_main_san)
hostsim: build/libhostsim.so build/libhostsim_ring8.so build/libhostsim_alpha.so build/libhostsim_region.so build/libhostsim_compose.so build/libhostsim_blend.so build/libhostsim_scale.so build/libhostsim_ycbcr.so build/libhostsim_orient.so build/libhostsim_lfframe.so build/liboracle_driver.so build/api_threads $(LAYOUTMAIN) $(SCALEMAIN) $(YCBCRMAIN) $(ORIENTMAIN) $(WIDESIM) $(WIDEMAIN) $(MODXYBSIM) $(MODXYBMAIN) $(COLOURSIM) $(COLOURMAIN) $(PATCHSIM) $(PATCHMAIN) $(NOISESIM) $(NOISEMAIN) $(UPSAMPLEMAIN) $(SPLINESIM) $(SPLINEMAIN)
# test-only glue: parses a stream with the product's host parser, takes the plan view and hands it to
# the CPU oracle (oracle/libj40oracle.so)
build/liboracle_driver.so: tests/oracle_driver.c build/libj40hip.so oracle/hotpath_oracle.c include/j40hip.h
	$(MAKE) -C oracle restatement
	gcc -O2 -fPIC -shared -Wall -o $@ tests/oracle_driver.c -Lbuild -Loracle -lj40hip -lj40oracle -Wl,-rpath,'$$ORIGIN' -Wl,-rpath,'$$ORIGIN/../oracle'

# test-only: many threads running the reference's public API sequence (dj40.c's) against the product library
build/api_threads: tests/api_threads.c include/j40.h build/libj40hip.so
	gcc -O2 -Wall -Wextra -pthread -Iinclude -o $@ tests/api_threads.c -Lbuild -lj40hip -Wl,-rpath,'$$ORIGIN'

# device functions compiled for the CPU, test infrastructure only (tests/hostsim)
HOSTSIM_SRC = tests/hostsim/hostsim.cpp $(SRC)/plan_build.cpp $(SRC)/plan_front.cpp $(SRC)/entropy.cpp $(SRC)/modular.cpp $(SRC)/tables.cpp $(SRC)/frame.cpp
HOSTSIM_FLAGS = -std=c++17 -O2 -fPIC -shared -ffp-contract=off -Wall -Wextra -Wno-unused-function -Wno-unknown-pragmas
build/libhostsim.so: $(HOSTSIM_SRC) $(HOSTSIM_HDR)
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(HOSTSIM_SRC) -lpthread
build/libhostsim_ring8.so: $(HOSTSIM_SRC) $(HOSTSIM_HDR)
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=8 -o $@ $(HOSTSIM_SRC) -lpthread

# the kept alpha channel of VarDCT frames on the CPU (tests/test_alpha.py): entropy decode, keep-mode trailer plan, device/alpha_dev.h's merge
ALPHASIM_SRC = tests/hostsim/alpha_sim.cpp $(SRC)/plan_build.cpp $(SRC)/plan_front.cpp $(SRC)/entropy.cpp $(SRC)/modular.cpp $(SRC)/tables.cpp $(SRC)/frame.cpp
build/libhostsim_alpha.so: $(ALPHASIM_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(ALPHASIM_SRC) -lpthread

# the Modular plan's layout (mod_layout.hpp) checked on the CPU (tests/test_mod_layout.py): the decodes of hostsim.cpp and alpha_sim.cpp as a
# program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
LAYOUTMAIN_SRC = tests/hostsim/mod_layout_main.cpp tests/hostsim/alpha_sim.cpp $(HOSTSIM_SRC)
LAYOUTMAIN_FLAGS = $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING)
build/mod_layout_main: $(LAYOUTMAIN_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(LAYOUTMAIN_FLAGS) -o $@ $(LAYOUTMAIN_SRC) -lpthread
build/mod_layout_main_san: $(LAYOUTMAIN_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(LAYOUTMAIN_FLAGS) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(LAYOUTMAIN_SRC) -lpthread

# region decode on the CPU (tests/test_region.py): device/region_dev.h's index, gather and crop functions over the host plan's varblock list
REGIONSIM_SRC = tests/hostsim/region_sim.cpp $(SRC)/plan_build.cpp $(SRC)/plan_front.cpp $(SRC)/entropy.cpp $(SRC)/modular.cpp $(SRC)/tables.cpp $(SRC)/frame.cpp
build/libhostsim_region.so: $(REGIONSIM_SRC) $(wildcard $(SRC)/device/*.h) $(wildcard $(SRC)/*.hpp) include/j40hip.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(REGIONSIM_SRC) -lpthread

# LF frames on the CPU (tests/test_lf_frames.py): device/lf_frame_dev.h's gather, LF index and block-context functions over the host plan
LFFRAMESIM_SRC = tests/hostsim/lf_frame_sim.cpp $(SRC)/plan_build.cpp $(SRC)/plan_front.cpp $(SRC)/entropy.cpp $(SRC)/modular.cpp $(SRC)/tables.cpp $(SRC)/frame.cpp
build/libhostsim_lfframe.so: $(LFFRAMESIM_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(LFFRAMESIM_SRC) -lpthread

# frame composition on the CPU (tests/test_frames.py): device/compose_dev.h's row functions over a canvas in host memory
build/libhostsim_compose.so: tests/hostsim/compose_sim.cpp $(SRC)/device/compose_dev.h $(SRC)/device/region_dev.h $(SRC)/device/plan.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ tests/hostsim/compose_sim.cpp

# ... and its blend modes (tests/test_blend.py): device/compose_dev.h's blend_row, the float32 arithmetic uncontracted as on the device
build/libhostsim_blend.so: tests/hostsim/blend_sim.cpp $(SRC)/device/compose_dev.h $(SRC)/device/region_dev.h $(SRC)/device/plan.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ tests/hostsim/blend_sim.cpp

# reduced-size decode on the CPU (tests/test_scale.py): device/scale_dev.h's row function over an image in host memory ...
build/libhostsim_scale.so: tests/hostsim/scale_sim.cpp $(SRC)/device/scale_dev.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -o $@ tests/hostsim/scale_sim.cpp
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
SCALEMAIN_SRC = tests/hostsim/scale_main.cpp tests/hostsim/scale_sim.cpp
build/scale_main: $(SCALEMAIN_SRC) $(SRC)/device/scale_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -o $@ $(SCALEMAIN_SRC)
build/scale_main_san: $(SCALEMAIN_SRC) $(SRC)/device/scale_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(SCALEMAIN_SRC)

# YCbCr VarDCT frames on the CPU (tests/test_ycbcr.py): host parse with subsampled channels, the plan, hf_dev.h's subsampled entropy
# decode, the pixel stage into planes, device/ycbcr_dev.h's tail ...
YCBCRSIM_SRC = tests/hostsim/ycbcr_sim.cpp $(SRC)/plan_build.cpp $(SRC)/plan_front.cpp $(SRC)/entropy.cpp $(SRC)/modular.cpp $(SRC)/tables.cpp $(SRC)/frame.cpp
build/libhostsim_ycbcr.so: $(YCBCRSIM_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(YCBCRSIM_SRC) -lpthread
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
YCBCRMAIN_SRC = tests/hostsim/ycbcr_main.cpp $(YCBCRSIM_SRC)
build/ycbcr_main: $(YCBCRMAIN_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(YCBCRMAIN_SRC) -lpthread
build/ycbcr_main_san: $(YCBCRMAIN_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(YCBCRMAIN_SRC) -lpthread

# oriented output on the CPU (tests/test_orient.py): device/orient_dev.h's row and tile functions over an image in host memory ...
build/libhostsim_orient.so: tests/hostsim/orient_sim.cpp $(SRC)/device/orient_dev.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -o $@ tests/hostsim/orient_sim.cpp
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
ORIENTMAIN_SRC = tests/hostsim/orient_main.cpp tests/hostsim/orient_sim.cpp
build/orient_main: $(ORIENTMAIN_SRC) $(SRC)/device/orient_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -o $@ $(ORIENTMAIN_SRC)
build/orient_main_san: $(ORIENTMAIN_SRC) $(SRC)/device/orient_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(ORIENTMAIN_SRC)

# wide Modular frames on the CPU (tests/test_wide_modular.py): the Modular device functions instantiated with int32 samples over a plan
# laid out with guard bytes ...
WIDESIM_SRC = tests/hostsim/wide_sim.cpp $(SRC)/plan_build.cpp $(SRC)/plan_front.cpp $(SRC)/entropy.cpp $(SRC)/modular.cpp $(SRC)/tables.cpp $(SRC)/frame.cpp
build/libwidesim.so: $(WIDESIM_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(WIDESIM_SRC) -lpthread
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
WIDEMAIN_SRC = tests/hostsim/wide_main.cpp $(WIDESIM_SRC)
build/wide_main: $(WIDEMAIN_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(WIDEMAIN_SRC) -lpthread
build/wide_main_san: $(WIDEMAIN_SRC) $(HOSTSIM_HDR) include/j40hip.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(WIDEMAIN_SRC) -lpthread

# Modular frames of XYB images on the CPU (tests/test_modular_xyb.py): device/modular_xyb_dev.h's lane functions over planes in host memory ...
MODXYBSIM_SRC = tests/hostsim/modular_xyb_sim.cpp $(SRC)/tables.cpp
build/libhostsim_modxyb.so: $(MODXYBSIM_SRC) $(HOSTSIM_HDR)
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(MODXYBSIM_SRC)
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
MODXYBMAIN_SRC = tests/hostsim/modular_xyb_main.cpp $(MODXYBSIM_SRC)
build/modular_xyb_main: $(MODXYBMAIN_SRC) $(HOSTSIM_HDR)
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(MODXYBMAIN_SRC)
build/modular_xyb_main_san: $(MODXYBMAIN_SRC) $(HOSTSIM_HDR)
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(MODXYBMAIN_SRC)

# the colour mode on the CPU (tests/test_colour.py): device/colour_dev.h's tail and colour_space.hpp's curves and threshold tables over planes in host memory ...
COLOURSIM_SRC = tests/hostsim/colour_sim.cpp
build/libhostsim_colour.so: $(COLOURSIM_SRC) $(HOSTSIM_HDR)
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(COLOURSIM_SRC) -lpthread
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
COLOURMAIN_SRC = tests/hostsim/colour_main.cpp $(COLOURSIM_SRC)
build/colour_main: $(COLOURMAIN_SRC) $(HOSTSIM_HDR)
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -o $@ $(COLOURMAIN_SRC) -lpthread
build/colour_main_san: $(COLOURMAIN_SRC) $(HOSTSIM_HDR)
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -DJ40_LANE_EV_FLUSH=$(EVENT_RING) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(COLOURMAIN_SRC) -lpthread

# patches on the CPU (tests/test_patches.py): device/patch_dev.h's lane function and tile binning over planes in host memory ...
build/libhostsim_patches.so: tests/hostsim/patch_sim.cpp $(SRC)/device/patch_dev.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -o $@ tests/hostsim/patch_sim.cpp
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
PATCHMAIN_SRC = tests/hostsim/patch_main.cpp tests/hostsim/patch_sim.cpp
build/patch_main: $(PATCHMAIN_SRC) $(SRC)/device/patch_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -o $@ $(PATCHMAIN_SRC)
build/patch_main_san: $(PATCHMAIN_SRC) $(SRC)/device/patch_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(PATCHMAIN_SRC)

# photon noise on the CPU (tests/test_noise.py): device/noise_dev.h's generator, jumped fill and tile functions over planes in host memory ...
build/libhostsim_noise.so: tests/hostsim/noise_sim.cpp $(SRC)/device/noise_dev.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -o $@ tests/hostsim/noise_sim.cpp
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
NOISEMAIN_SRC = tests/hostsim/noise_main.cpp tests/hostsim/noise_sim.cpp
build/noise_main: $(NOISEMAIN_SRC) $(SRC)/device/noise_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -o $@ $(NOISEMAIN_SRC)
build/noise_main_san: $(NOISEMAIN_SRC) $(SRC)/device/noise_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(NOISEMAIN_SRC)

# splines on the CPU (tests/test_splines.py): device/spline_dev.h's dequantisation, binning and lane function over planes in host memory ...
build/libhostsim_splines.so: tests/hostsim/spline_sim.cpp $(SRC)/device/spline_dev.h
	@mkdir -p build
	$(CXX) $(HOSTSIM_FLAGS) -o $@ tests/hostsim/spline_sim.cpp
# ... and as a program of its own, plain and with the host sanitizers (an executable: never loaded into Python)
SPLINEMAIN_SRC = tests/hostsim/spline_main.cpp tests/hostsim/spline_sim.cpp
build/spline_main: $(SPLINEMAIN_SRC) $(SRC)/device/spline_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -o $@ $(SPLINEMAIN_SRC)
build/spline_main_san: $(SPLINEMAIN_SRC) $(SRC)/device/spline_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(SPLINEMAIN_SRC)

# upsampling on the CPU (tests/test_upsampling.py): device/upsample_dev.h's rule and tile functions as a program of its own, plain and with
# the host sanitizers (an executable: never loaded into Python; the library's j40hip_kat_host_upsample is the same code for the tests' numpy)
build/upsample_main: tests/hostsim/upsample_main.cpp $(SRC)/device/upsample_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -o $@ tests/hostsim/upsample_main.cpp
build/upsample_main_san: tests/hostsim/upsample_main.cpp $(SRC)/device/upsample_dev.h
	@mkdir -p build
	$(CXX) $(filter-out -fPIC -shared,$(HOSTSIM_FLAGS)) -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ tests/hostsim/upsample_main.cpp

build/jxlsynth: tools/jxlsynth.cpp $(wildcard tools/*.hpp) $(SRC)/tables.cpp $(SRC)/device/special8_dev.h $(SRC)/device/idct_dev.h
	@mkdir -p build
	$(CXX) -O2 -std=c++17 -ffp-contract=off -Wall -Wextra -Wno-unused-function -Wno-unknown-pragmas -o $@ $< $(SRC)/tables.cpp

clean:
	rm -rf build
	$(MAKE) -C oracle clean
