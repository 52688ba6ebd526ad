"""Registry of the TIMING ENTRIES of the C ABI (include/spmv_acc.h, "measurement helper") and of the forms their y reset takes: every published
figure -- bench.py's `value`, `ms_per_step`, the per-launch fractions, the cold-cache column, the copy ceiling -- is read from these entries, and a
reset that did not happen, or a flush copy that writes where it should not, changes a figure without failing anything.  So each entry names the GPU
tests (tests/test_gpu_timing_entries.py) that call it and pin what it leaves behind, and each condition of spmv_acc_amd/csrc/c_api.cpp that selects
a form of the reset names the tests that cross it.

tests/test_timing_entries_host.py checks, without a GPU, that
  * every `spmv_acc_time_*` / `spmv_acc_copy_ceiling_gbs` prototype of the header has an entry here (a NEW timing entry fails the CPU suite until
    someone registers the tests that call it), and nothing here names a prototype the header no longer has,
  * every test named here exists in the GPU file, and the GPU file names the entry,
  * every `pattern` of RESET_FORMS still matches c_api.cpp (a rewritten protocol body has to re-register what crosses it).
"""

GPU_FILE = "tests/test_gpu_timing_entries.py"
SOURCE = "spmv_acc_amd/csrc/c_api.cpp"
HEADER = "include/spmv_acc.h"
PROTOTYPE = r"^(?:int|double)\s+(spmv_acc_time_\w+|spmv_acc_copy_ceiling_gbs)\s*\("

_PER_LAUNCH = ["test_per_launch_entries_restore_y_line_enhance", "test_per_launch_entries_restore_y_flat_and_adaptive",
               "test_per_launch_entries_without_y0_accumulate", "test_bad_arguments_leave_everything_untouched",
               "test_unknown_strategy_id_is_refused_before_anything_is_written", "test_zero_rows_launch_nothing"]

# C prototype -> the GPU tests that call it
TIMING_ENTRIES = {
    "spmv_acc_time_spmv": _PER_LAUNCH + ["test_reset_switches_in_a_fresh_process", "test_per_launch_entries_on_a_side_stream"],
    "spmv_acc_time_spmv_events": _PER_LAUNCH + ["test_reset_switches_in_a_fresh_process", "test_per_launch_entries_on_a_side_stream"],
    "spmv_acc_time_spmv_cold": _PER_LAUNCH + ["test_cold_flush_overwrites_its_second_half_with_its_first", "test_cold_entry_refuses_a_bad_flush_buffer",
                                              "test_reset_switches_in_a_fresh_process", "test_per_launch_entries_on_a_side_stream"],
    "spmv_acc_time_spmv_kernels": _PER_LAUNCH + ["test_reset_switches_in_a_fresh_process", "test_per_launch_entries_on_a_side_stream"],
    "spmv_acc_time_spmv_total": ["test_total_and_region_accumulate", "test_bad_arguments_leave_everything_untouched",
                                 "test_unknown_strategy_id_is_refused_before_anything_is_written", "test_zero_rows_launch_nothing"],
    "spmv_acc_time_spmv_region": ["test_total_and_region_accumulate", "test_region_refuses_a_plan_that_was_not_settled",
                                  "test_bad_arguments_leave_everything_untouched", "test_unknown_strategy_id_is_refused_before_anything_is_written",
                                  "test_zero_rows_launch_nothing"],
    "spmv_acc_copy_ceiling_gbs": ["test_copy_ceiling_copies_exactly_its_bytes", "test_copy_ceiling_refusals_write_nothing"],
}

# (what, regex that must match c_api.cpp, tests that cross it, what it selects)
RESET_FORMS = [
    ("per-launch reset: alignment test",
     r"const bool kernel_copy = !reset_memcpy && reinterpret_cast<uintptr_t>\(dy\) % 16 == 0 && reinterpret_cast<uintptr_t>\(d_y0\) % 16 == 0;",
     ["test_per_launch_entries_restore_y_line_enhance", "test_per_launch_entries_restore_y_flat_and_adaptive"],
     "y and y0 both 16-byte aligned: the 16-byte copy kernel; else hipMemcpyAsync"),
    ("per-launch reset: the 16-byte body",
     r"const size_t body = kernel_copy \? ybytes / 16 \* 16 : 0;\s*\n\s*if \(body\) launch_stream_copy\(st, dy, d_y0, static_cast<long long>\(body\), reset_nt\);",
     ["test_per_launch_entries_restore_y_line_enhance"], "m = 1: no body at all; m = 2: exactly one unit"),
    ("per-launch reset: odd-m tail launch",
     r"if \(body < ybytes && kernel_copy\)[^\n]*\n\s*hipLaunchKernelGGL\(copy_doubles_kernel, dim3\(1\), dim3\(64\), 0, st, dy \+ body / 8, d_y0 \+ body / 8,",
     ["test_per_launch_entries_restore_y_line_enhance", "test_per_launch_entries_restore_y_flat_and_adaptive"],
     "odd m: the last double by a one-workgroup copy_doubles_kernel (m = 4097, 3, 1)"),
    ("per-launch reset: hipMemcpyAsync fallback",
     r"else if \(body < ybytes\)\s*\n\s*\(void\)hipMemcpyAsync\(dy, d_y0, ybytes, hipMemcpyDeviceToDevice, st\);",
     ["test_per_launch_entries_restore_y_line_enhance", "test_per_launch_entries_restore_y_flat_and_adaptive", "test_reset_switches_in_a_fresh_process"],
     "y or y0 at 8 mod 16, or SPMV_ACC_RESET_MEMCPY=1"),
    ("kernel-clock reset: alignment and odd-m test",
     r"if \(ybytes % 16 == 0 && reinterpret_cast<uintptr_t>\(dy\) % 16 == 0 && reinterpret_cast<uintptr_t>\(d_y0\) % 16 == 0\)\s*\n"
     r"\s*launch_stream_copy\(st, dy, d_y0, static_cast<long long>\(ybytes\), reset_nt_copy\(\)\);\s*\n\s*else\s*\n"
     r"\s*\(void\)hipMemcpyAsync\(dy, d_y0, ybytes, hipMemcpyDeviceToDevice, st\);",
     ["test_per_launch_entries_restore_y_line_enhance", "test_per_launch_entries_restore_y_flat_and_adaptive"],
     "spmv_acc_time_spmv_kernels: odd m goes to hipMemcpyAsync, not to a tail kernel"),
    ("cold entry: flush buffer alignment test",
     r"if \(!d_flush \|\| flush_bytes < 32 \|\| reinterpret_cast<uintptr_t>\(d_flush\) % 16 != 0\)",
     ["test_cold_entry_refuses_a_bad_flush_buffer"], "NULL, fewer than 32 bytes, or a base off 16: refused"),
    ("cold entry: flush copy",
     r"const long long half = flush_bytes / 2 / 16 \* 16;\s*\n\s*launch_stream_copy\(st, static_cast<char \*>\(d_flush\) \+ half, d_flush, half, /\*non_temporal=\*/false\);",
     ["test_cold_flush_overwrites_its_second_half_with_its_first"], "bytes [half, 2 * half) <- bytes [0, half), nothing else"),
    ("accumulation without y0", r"if \(d_y0\) \{\s*\n\s*const size_t body",
     ["test_per_launch_entries_without_y0_accumulate"], "d_y0 == NULL: no reset, y accumulates over the launches"),
    ("region: the plan was not settled", r"if \(rc == kOk && plan_work_count\(\) != work0\) \{",
     ["test_region_refuses_a_plan_that_was_not_settled"], "plan work inside the timed region is reported, the time is still written"),
    ("SPMV_ACC_RESET_MEMCPY", r'std::getenv\("SPMV_ACC_RESET_MEMCPY"\)', ["test_reset_switches_in_a_fresh_process"], "read once per process"),
    ("SPMV_ACC_RESET_NT", r'std::getenv\("SPMV_ACC_RESET_NT"\)', ["test_reset_switches_in_a_fresh_process"], "read once per process (two readers)"),
]
