# oracle/refhost.mk -- the REFERENCE's own host code over this repository's C ABI (TEST INFRASTRUCTURE ONLY).
#
#   make -f refhost.mk
#             _ref/libhavac_refhost.so         host/Havac.cpp, host/phmm/PhmmPreprocessor.cpp,
#                                               host/sequence/SequencePreprocessor.cpp and
#                                               PhmmReprojection/PhmmReprojection.cpp of the reference, compiled from
#                                               where they lie (build container only; the .so travels to the GPU box,
#                                               the sources never do), linked to havac_amd/libhavac_dev.so
#             _ref/libssv_ref2.so              host/test/Ssv.cpp (HitsFromSsv, the reference's per-(model, record)
#                                               CPU SSV) the same way; used once, to capture tests/golden/g8_*.npz
#
# The wrappers are tests/refhost/*_wrap.cpp; tests/refhost/binding.py loads the results.
# Substitutions (see tests/refhost/refhost_wrap.cpp for the why of each):
#   -DHAVAC_HW_CLIENT_HPP -include integration/HavacHwClient.hpp   the reference's XRT client header is skipped by its
#                                                                  own include guard, the binding is force-included
#   -DHAVAC_HLS_PUBLIC_DEFINES_H -DNUM_CELL_PROCESSORS=12288       device/PublicDefines.h needs Vitis' <ap_int.h>;
#                                                                  12288 = 16 * 768, PublicDefines.h:18-22
#   -I havac_amd/csrc/host  (searched for <FastaVector.h>, <p7HmmReader.h> only: every other include of the reference's
#                            files is a quoted, relative one and resolves inside /root/reference)
# The reference builds its C++ without an optimisation level or -march (CMakeLists.txt:66 sets C flags only): -O0 here.
# No stand-in header is written for anything.
REFERENCE ?= /root/reference
CXX ?= g++
ROOT = ..
HOST = $(ROOT)/havac_amd/csrc/host
OUT  = _ref
WRAP = $(ROOT)/tests/refhost
SUBST = -DHAVAC_HW_CLIENT_HPP -include $(ROOT)/integration/HavacHwClient.hpp \
        -DHAVAC_HLS_PUBLIC_DEFINES_H -DNUM_CELL_PROCESSORS=12288
FLAGS = -O0 -g0 -fPIC -pthread -std=c++17 -I$(ROOT)/include -I$(HOST)
REF_SRC = $(REFERENCE)/host/Havac.cpp $(REFERENCE)/host/phmm/PhmmPreprocessor.cpp \
          $(REFERENCE)/host/sequence/SequencePreprocessor.cpp $(REFERENCE)/PhmmReprojection/PhmmReprojection.cpp
READERS = $(HOST)/FastaVector.cpp $(HOST)/p7HmmReader.cpp

all: $(OUT)/libhavac_refhost.so $(OUT)/libssv_ref2.so

# -Bsymbolic: the reference's Havac / HavacHit / SequencePreprocessor / PhmmPreprocessor have the same names as the
# product's classes in libhavac.so; each library binds to its own copies even when a test loads both.
$(OUT)/libhavac_refhost.so: $(WRAP)/refhost_wrap.cpp $(REF_SRC) $(READERS) $(ROOT)/integration/HavacHwClient.hpp $(ROOT)/include/havac_dev.h
	mkdir -p $(OUT)
	$(CXX) $(FLAGS) $(SUBST) -I$(REFERENCE)/host -shared -Wl,-Bsymbolic -o $@ $(WRAP)/refhost_wrap.cpp $(REF_SRC) $(READERS) \
	    -L$(ROOT)/havac_amd -lhavac_dev -Wl,-rpath,'$$ORIGIN/../../havac_amd'

$(OUT)/libssv_ref2.so: $(WRAP)/ssv_ref2_wrap.cpp $(REFERENCE)/host/test/Ssv.cpp $(REFERENCE)/PhmmReprojection/PhmmReprojection.cpp $(READERS)
	mkdir -p $(OUT)
	$(CXX) $(FLAGS) -I$(REFERENCE)/host/test -shared -Wl,-Bsymbolic -o $@ $(WRAP)/ssv_ref2_wrap.cpp \
	    $(REFERENCE)/host/test/Ssv.cpp $(REFERENCE)/PhmmReprojection/PhmmReprojection.cpp $(READERS)

clean:
	rm -f $(OUT)/libhavac_refhost.so $(OUT)/libssv_ref2.so

.PHONY: all clean
