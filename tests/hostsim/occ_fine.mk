# test-only host build of the lane math of ssde_path_occupancy_fine (see hostsim_occ_fine.cpp): make -f occ_fine.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
all: libhostsim_occ_fine.so
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_occ_fine.so: hostsim_occ_fine.cpp hostsim_occ_fine.hpp hostsim_records.hpp $(C)/ssde_bridge.hpp $(C)/ssde_occ.hpp $(C)/ssde_smooth_plan.hpp $(C)/ssde_predict.hpp $(C)/ssde_draws.hpp $(C)/ssde_smooth.hpp $(C)/ssde_dense.hpp $(C)/ssde_math.hpp
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
