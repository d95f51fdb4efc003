# test-only host build of the lane math and tile plan of ssde_path_proximity (see hostsim_prox.cpp), and the stand-alone program that
# runs them under AddressSanitizer / UndefinedBehaviorSanitizer (prox_san.cpp): make -f prox.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
DEPS := hostsim_prox.hpp $(C)/ssde_prox.hpp $(C)/ssde_path.hpp $(C)/ssde_occ.hpp $(C)/ssde_draws.hpp $(C)/ssde_smooth.hpp $(C)/ssde_dense.hpp $(C)/ssde_math.hpp
all: libhostsim_prox.so prox_san
# (through a temporary name: a test run may load the library while another builds it)
libhostsim_prox.so: hostsim_prox.cpp $(DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
# (the sanitizers' runtimes linked into the program: it runs as it stands, with nothing to load beside it)
prox_san: prox_san.cpp $(DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
