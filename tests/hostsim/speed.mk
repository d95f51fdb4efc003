# test-only host build of the lane math of ssde_path_speed (see hostsim_speed.cpp), and the stand-alone program that runs it under
# AddressSanitizer / UndefinedBehaviorSanitizer (speed_san.cpp): make -f speed.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
DEPS := hostsim_speed.hpp hostsim_records.hpp $(C)/ssde_speed.hpp $(C)/ssde_predict.hpp $(C)/ssde_draws.hpp $(C)/ssde_smooth.hpp $(C)/ssde_dense.hpp $(C)/ssde_math.hpp
all: libhostsim_speed.so speed_san
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_speed.so: hostsim_speed.cpp $(DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
# (the sanitizers' runtimes linked into the program: it runs as it stands, with nothing to load beside it; under their
# instrumentation g++ suspects the empty tangent array of DualN<0> in ssde_dense.hpp of being read when a DualN is returned by value: the -Wno- flags)
speed_san: speed_san.cpp $(DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -Wno-uninitialized -Wno-maybe-uninitialized -Wno-misleading-indentation -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
