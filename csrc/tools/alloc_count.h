// Hooks of the counting allocator (csrc/tools/alloc_count.cc). The stress
// driver is linked with it only in the `--stress-count` flavour; everywhere
// else these weak symbols are null and the driver skips the calls.
#pragma once

#include <cstdint>
#include <cstdio>

namespace xsched::alloc_count {

// Switch counting on or off (off at start: warm-up waves are not counted).
__attribute__((weak)) void enable(bool on);
// One line per thread name (threads sharing a name are summed), the
// scheduling thread's `new_per_bound_pod`, and with XSCHED_ALLOC_STACKS=1 the
// top call stacks of the thread XSCHED_ALLOC_THREAD names (default xs-sched).
__attribute__((weak)) void report(std::FILE* out, uint64_t bound_pods);

}  // namespace xsched::alloc_count
