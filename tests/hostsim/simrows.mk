# test-only host build of the lane math of ssde_simulate_rows (see hostsim_simrows.cpp), and the stand-alone program that runs it
# under AddressSanitizer / UndefinedBehaviorSanitizer (simrows_san.cpp): make -f simrows.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
DEPS := hostsim_simrows.hpp $(C)/ssde_simrows.hpp $(C)/ssde_philox.hpp $(C)/ssde_bands.hpp $(C)/ssde_math.hpp
all: libhostsim_simrows.so simrows_san
# (through a temporary name: a test run may load the library while another builds it; -ffp-contract=off: the header says where an
# fma is, and nothing else becomes one)
libhostsim_simrows.so: hostsim_simrows.cpp $(DEPS)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -ffp-contract=off -shared -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
# (the sanitizers' runtimes linked into the program: it runs as it stands, with nothing to load beside it)
simrows_san: simrows_san.cpp $(DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
