# The launch-lane bookkeeping (odp_amd/csrc/lanes.h, plain C) against its
# brute-force model, under AddressSanitizer + UBSan, no GPU. Run by
# tests/test_lanes.py. Usage: make -C tests/c -f lanes_model.mk
CSRC := ../../odp_amd/csrc

lanes_model.asan: lanes_model.cpp $(CSRC)/lanes.h
	$(CXX) -std=c++17 -g -O1 -fno-omit-frame-pointer -Wall -Wextra \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<

clean:
	rm -f lanes_model.asan

.PHONY: clean
