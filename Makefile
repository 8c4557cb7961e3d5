# malva-hip build.  Everything is built in-tree so the artefacts travel with the
# repo snapshot to the GPU box; none of them is committed (.gitignore).
#
#   make lib      HIP kernels + C-ABI       -> malva_amd/lib/libmalva_hip.so   (hipcc, gfx950)
#   make cli      C++17 host driver         -> bin/malva-geno
#   make oracle   CPU restatement (checker) -> oracle/libmalva_oracle.so       (gcc)
#   make ref      the reference's own vendored xxhash.c, compiled where it lies
#                 under /root/reference     -> oracle/_ref/libxxhash_ref.so    (only when the reference is present)

HIPCC      ?= /opt/rocm/bin/hipcc
CC         ?= gcc
CXX        ?= g++
ARCH       ?= gfx950
REFERENCE  ?= /root/reference
# zstd for the reference's index container: the image has the runtime library system-wide and the header only under
# /opt/conda (searched AFTER the system directories, so nothing else is taken from there)
ZSTD_INC   ?= /opt/conda/include
ZSTD_LIB   ?= /usr/lib/x86_64-linux-gnu/libzstd.so.1

HIPFLAGS   := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Iinclude -Imalva_amd/csrc \
              -Wall -Wno-unused-function -Wno-unused-value -fvisibility=hidden
CSRC       := $(wildcard malva_amd/csrc/*.hip)
CHDR       := $(wildcard malva_amd/csrc/*.h) $(wildcard include/*.h)
HOSTSRC    := $(wildcard malva_amd/host/*.cpp)
HOSTHDR    := $(wildcard malva_amd/host/*.hpp)

all: lib oracle ref cli

lib: malva_amd/lib/libmalva_hip.so
malva_amd/lib/libmalva_hip.so: $(CSRC) $(CHDR)
	@mkdir -p malva_amd/lib
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(CSRC)

cli: bin/malva-geno
bin/malva-geno: $(HOSTSRC) $(HOSTHDR) malva_amd/lib/libmalva_hip.so
	@mkdir -p bin
	$(CXX) -std=c++17 -O2 -Wall -pthread -Iinclude -Imalva_amd/host -idirafter $(ZSTD_INC) -o $@ $(HOSTSRC) \
	    -Lmalva_amd/lib -lmalva_hip -lz $(ZSTD_LIB) -Wl,-rpath,'$$ORIGIN/../malva_amd/lib'

oracle: oracle/libmalva_oracle.so
oracle/libmalva_oracle.so: oracle/malva_oracle.c
	$(CC) -O2 -ffp-contract=off -fPIC -shared -fvisibility=hidden -Wall -pthread -o $@ $< -lm

# The reference build: its own xxhash.c (which includes its own xxhash.h),
# untouched, straight from the read-only checkout.  Skipped on machines that do
# not have the reference (the GPU box); the prebuilt .so travels instead.
ref:
	@if [ -f $(REFERENCE)/xxhash.c ]; then \
	    mkdir -p oracle/_ref && \
	    $(CC) -O2 -fPIC -shared -o oracle/_ref/libxxhash_ref.so $(REFERENCE)/xxhash.c && \
	    echo "built oracle/_ref/libxxhash_ref.so from $(REFERENCE)/xxhash.c"; \
	else echo "reference not present: keeping prebuilt oracle/_ref (if any)"; fi

# the microbenchmark behind DESIGN.md's bound for the filter kernel (run it on an MI355X)
microbench: bin/l2_gather_bench bin/ticket_gate_bench
bin/l2_gather_bench: tools/l2_gather_bench.hip
	@mkdir -p bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
# the bare access pattern of the ticket form's pass two
bin/ticket_gate_bench: tools/ticket_gate_bench.hip
	@mkdir -p bin
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-value -o $@ $<

# the host side of --cohort-priors (option values, --priors-out; --prior-groups' scratch streams), of the cohort's outputs (--site-stats, --ld, --ibd and --grm in programs of their own) and of the panel batches and their text under
# AddressSanitizer and UBSan: stand-alone programs, run on the CPU.  The last one is a batch's device calls and the pipeline around them
# (host/call_worker.hpp) against an ABI of its own, without libmalva_hip; it runs a second time under ThreadSanitizer.  Last, the command line
# (host/options.hpp) against the records of the parser it replaced, and the host half of `pca` (host/pca.hpp, csrc/pca_plan.h)
sanitize-host: bin/cohort_priors_host_check bin/cohort_priors_groups_host_check bin/cohort_out_host_check bin/site_table_host_check bin/ld_out_host_check bin/ibd_out_host_check bin/grm_out_host_check \
               bin/call_batch_host_check bin/call_worker_host_check bin/call_worker_host_check_tsan bin/options_host_check bin/pca_host_check
	bin/cohort_priors_host_check bin
	bin/cohort_priors_groups_host_check bin
	bin/cohort_out_host_check bin
	bin/site_table_host_check bin
	bin/ld_out_host_check bin
	bin/ibd_out_host_check bin
	bin/grm_out_host_check bin
	bin/call_batch_host_check
	bin/call_worker_host_check bin
	bin/call_worker_host_check_tsan bin
	bin/options_host_check
	bin/pca_host_check bin
bin/cohort_priors_host_check: tools/cohort_priors_host_check.cpp malva_amd/host/cohort_priors.hpp malva_amd/host/part_file.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $<
bin/cohort_priors_groups_host_check: tools/cohort_priors_groups_host_check.cpp malva_amd/host/cohort_priors.hpp malva_amd/host/part_file.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $<
bin/cohort_out_host_check: tools/cohort_out_host_check.cpp malva_amd/host/cohort_out.hpp malva_amd/host/part_file.hpp malva_amd/host/bcf_out.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $< -lz
bin/site_table_host_check: tools/site_table_host_check.cpp malva_amd/host/cohort_out.hpp malva_amd/host/part_file.hpp malva_amd/host/bcf_out.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $< -lz
bin/ld_out_host_check: tools/ld_out_host_check.cpp malva_amd/host/cohort_out.hpp malva_amd/host/part_file.hpp malva_amd/host/bcf_out.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $< -lz
bin/ibd_out_host_check: tools/ibd_out_host_check.cpp malva_amd/host/cohort_out.hpp malva_amd/host/part_file.hpp malva_amd/host/bcf_out.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $< -lz
bin/grm_out_host_check: tools/grm_out_host_check.cpp tools/grm_host_loop.cpp malva_amd/host/cohort_out.hpp malva_amd/host/part_file.hpp malva_amd/host/bcf_out.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $< -lz
# the GRM's definition as a one-core loop, for tools/grm_bench.py (which loads it) and on its own
grm-tools: bin/libgrm_host_loop.so
bin/libgrm_host_loop.so: tools/grm_host_loop.cpp
	@mkdir -p bin
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fPIC -shared -o $@ $<
bin/call_batch_host_check: tools/call_batch_host_check.cpp tools/host_check_util.hpp malva_amd/host/panel_batch.hpp malva_amd/host/call_text.hpp malva_amd/host/block.hpp \
                           malva_amd/host/io.hpp malva_amd/host/bcf_out.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $< -lz
bin/call_worker_host_check: tools/call_worker_host_check.cpp tools/host_check_util.hpp $(HOSTHDR) include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $< -lz
bin/call_worker_host_check_tsan: tools/call_worker_host_check.cpp tools/host_check_util.hpp $(HOSTHDR) include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -pthread -fsanitize=thread -Imalva_amd/host -o $@ $< -lz
# the command line (host/options.hpp, usage.hpp) against the records of tests/golden/options_cases.jsonl
bin/options_host_check: tools/options_host_check.cpp malva_amd/host/options.hpp malva_amd/host/usage.hpp malva_amd/host/cohort_priors.hpp malva_amd/host/part_file.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $<
# the readers, writers and parser of `malva-geno pca`, the block geometry and the small Jacobi solver
bin/pca_host_check: tools/pca_host_check.cpp malva_amd/host/pca.hpp malva_amd/csrc/pca_plan.h malva_amd/host/cohort_out.hpp malva_amd/host/part_file.hpp malva_amd/host/bcf_out.hpp include/malva_hip.h
	@mkdir -p bin
	$(CXX) -std=c++17 -O1 -g -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Imalva_amd/host -o $@ $< -lz

clean:
	rm -rf malva_amd/lib bin oracle/libmalva_oracle.so oracle/_ref

.PHONY: all lib cli oracle ref microbench sanitize-host grm-tools clean
