# the pileup entries' host side (mgl_amd/csrc/sw_pileup.cpp) under ASan + UBSan against the fake HIP runtime (fake_hip/): a target beside
# host-san that reuses Makefile's own source list, flags and checker object (it is included, not copied); pileup_san_driver.cpp stands
# where host_san_driver.cpp stands there, and where the kernels of sw_pileup.hip stand.  Never shipped.
#   make -C tests/cpp -f pileup_san.mk pileup-san
include $(dir $(abspath $(lastword $(MAKEFILE_LIST))))Makefile
PILEUP_SRCS := $(HERE)pileup_san_driver.cpp $(CSRC)/sw_pileup.cpp $(filter-out $(HERE)host_san_driver.cpp,$(SAN_SRCS))
$(HERE)pileup_san_asan: $(PILEUP_SRCS) $(CSRC)/sw_pileup.h $(CSRC)/sw_describe.h $(SAN_DEPS) $(HERE)sw_oracle_plain.o
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(PILEUP_SRCS) $(HERE)sw_oracle_plain.o
pileup-san: $(HERE)pileup_san_asan
	ASAN_OPTIONS=detect_leaks=1 $(HERE)pileup_san_asan
.PHONY: pileup-san
