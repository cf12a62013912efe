# the insertions and genotype entries' host side (mgl_amd/csrc/sw_calls.cpp) under ASan + UBSan against the fake HIP runtime (fake_hip/):
# a target beside host-san that reuses Makefile's own source list, flags and checker object (it is included, not copied);
# calls_san_driver.cpp stands where host_san_driver.cpp stands there, and where the kernels of sw_calls.hip stand.  Never shipped.
#   make -C tests/cpp -f calls_san.mk calls-san
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
CALLS_SRCS := $(HERE)calls_san_driver.cpp $(CSRC)/sw_calls.cpp $(filter-out $(HERE)host_san_driver.cpp,$(SAN_SRCS))
$(HERE)calls_san_asan: $(CALLS_SRCS) $(CSRC)/sw_calls.h $(CSRC)/sw_pileup.h $(CSRC)/sw_describe.h $(SAN_DEPS) $(HERE)sw_oracle_plain.o
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(CALLS_SRCS) $(HERE)sw_oracle_plain.o
calls-san: $(HERE)calls_san_asan
	ASAN_OPTIONS=detect_leaks=1 $(HERE)calls_san_asan
.PHONY: calls-san
