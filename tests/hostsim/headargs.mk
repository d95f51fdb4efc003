# test-only host build of the lag-path head's argument block (see hostsim_headargs.cpp): make -f headargs.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
ROCM_PATH ?= /opt/rocm
all: libhostsim_headargs.so
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_headargs.so: hostsim_headargs.cpp $(C)/ssde_device.hpp $(C)/ssde_gain_feed.hpp $(C)/ssde_math.hpp
	$(CXX) -O2 -std=c++17 -fPIC -Wall -D__HIP_PLATFORM_AMD__ -I$(ROCM_PATH)/include -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
