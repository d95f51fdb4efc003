# test-only host build of the lane math of ssde_predict_draws (see hostsim_predict_draws.cpp): make -f predict_draws.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
all: libhostsim_predict_draws.so
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_predict_draws.so: hostsim_predict_draws.cpp hostsim_records.hpp $(C)/ssde_bridge.hpp $(C)/ssde_smooth_plan.hpp $(C)/ssde_predict.hpp $(C)/ssde_draws.hpp $(C)/ssde_smooth.hpp $(C)/ssde_dense.hpp $(C)/ssde_math.hpp
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
