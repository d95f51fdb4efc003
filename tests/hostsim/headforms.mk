# test-only: the host forms of the lag-path head (csrc/ssde_headforms.hpp) as a stand-alone program under AddressSanitizer /
# UndefinedBehaviorSanitizer (headforms_san.cpp): make -f headforms.mk
CXX ?= g++
C := ../../smoothsde_amd/csrc
DEPS := $(C)/ssde_headforms.hpp $(C)/ssde_math.hpp
all: headforms_san
# (the sanitizers' runtimes linked into the program: it runs as it stands, with nothing to load beside it; through a temporary name:
# a test run may start the program while another builds it; -Wno-psabi: the header's four-double vector type never crosses a call)
headforms_san: headforms_san.cpp $(DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -Wno-psabi -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@.$$$$.tmp $< && mv $@.$$$$.tmp $@
