# the expand and classify entries' host side (mgl_amd/csrc/sw_lines.cpp) under ASan + UBSan against the fake HIP runtime (fake_hip/):
# a target beside host-san that reuses Makefile's own source list, flags and checker object (it is included, not copied);
# lines_san_driver.cpp stands where host_san_driver.cpp stands there, and where the kernels of sw_lines.hip stand.  Never shipped.
#   make -C tests/cpp -f lines_san.mk lines-san
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
LINES_SRCS := $(HERE)lines_san_driver.cpp $(CSRC)/sw_lines.cpp $(filter-out $(HERE)host_san_driver.cpp,$(SAN_SRCS))
$(HERE)lines_san_asan: $(LINES_SRCS) $(CSRC)/sw_lines.h $(SAN_DEPS) $(HERE)sw_oracle_plain.o
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(LINES_SRCS) $(HERE)sw_oracle_plain.o
lines-san: $(HERE)lines_san_asan
	ASAN_OPTIONS=detect_leaks=1 $(HERE)lines_san_asan
.PHONY: lines-san
