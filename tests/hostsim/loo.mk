# test-only host build of the lane math of ssde_smooth_loo (see hostsim_loo.cpp), and the stand-alone program that runs it under
# AddressSanitizer / UndefinedBehaviorSanitizer (loo_san.cpp): make -f loo.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
DEPS := hostsim_loo.hpp hostsim_records.hpp $(C)/ssde_loo.hpp $(C)/ssde_predict.hpp $(C)/ssde_smooth.hpp $(C)/ssde_dense.hpp $(C)/ssde_math.hpp ../../include/ssde.h
all: libhostsim_loo.so loo_san
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_loo.so: hostsim_loo.cpp $(DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -Wno-misleading-indentation -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
# (the sanitizers' runtimes linked into the program: it runs as it stands, with nothing to load beside it; under their
# instrumentation g++ suspects the empty tangent array of DualN<0> in ssde_dense.hpp of being read when a DualN is returned by value: the -Wno- flags)
loo_san: loo_san.cpp $(DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -Wno-uninitialized -Wno-maybe-uninitialized -Wno-misleading-indentation -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
