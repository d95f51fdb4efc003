# test-only host build of the window geometry with the early bulk cut (see hostsim_headcut.cpp): make -f headcut.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
all: libhostsim_headcut.so
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_headcut.so: hostsim_headcut.cpp $(C)/ssde_windows.hpp $(C)/ssde_math.hpp
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
