# test-only host build of the lane math of ssde_path_occupancy (see hostsim_occ.cpp): make -f occ.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
all: libhostsim_occ.so
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_occ.so: hostsim_occ.cpp hostsim_records.hpp $(C)/ssde_occ.hpp $(C)/ssde_smooth_plan.hpp $(C)/ssde_predict.hpp $(C)/ssde_draws.hpp $(C)/ssde_smooth.hpp $(C)/ssde_dense.hpp $(C)/ssde_math.hpp
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
