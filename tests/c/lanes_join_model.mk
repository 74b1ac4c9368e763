# Joins of the launch-lane bookkeeping (odp_amd/csrc/lanes.h, plain C): the
# launch / join call patterns of a receive loop on vector clocks, under
# AddressSanitizer + UBSan, no GPU. Run by tests/test_counted_lanes.py.
# Usage: make -C tests/c -f lanes_join_model.mk
CSRC := ../../odp_amd/csrc

lanes_join_model.asan: lanes_join_model.cpp $(CSRC)/lanes.h
	$(CXX) -std=c++17 -g -O1 -fno-omit-frame-pointer -Wall -Wextra \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<

clean:
	rm -f lanes_join_model.asan

.PHONY: clean
