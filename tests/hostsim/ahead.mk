# test-only host build of the lane math and host plan of ssde_forecast_scores (see hostsim_ahead.cpp), and the stand-alone program
# that runs it under AddressSanitizer / UndefinedBehaviorSanitizer (ahead_san.cpp): make -f ahead.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
DEPS := hostsim_ahead.hpp hostsim_records.hpp $(C)/ssde_ahead.hpp $(C)/ssde_loo.hpp $(C)/ssde_smooth_plan.hpp $(C)/ssde_predict.hpp $(C)/ssde_smooth.hpp $(C)/ssde_dense.hpp $(C)/ssde_math.hpp ../../include/ssde.h
all: libhostsim_ahead.so ahead_san
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_ahead.so: hostsim_ahead.cpp $(DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -Wno-misleading-indentation -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
# (the sanitizers' runtimes linked into the program: it runs as it stands, with nothing to load beside it; the -Wno- flags as loo.mk)
ahead_san: ahead_san.cpp $(DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -Wno-uninitialized -Wno-maybe-uninitialized -Wno-misleading-indentation -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
