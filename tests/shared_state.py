"""What the contexts of one process share: every writable object with static storage in flo_amd/libflo_hip.so, with what
guards it. include/flo_hip.h promises that contexts are independent, one per host thread; each object here is a place where
two contexts' threads can meet, so each needs a reason why that is safe. tests/test_shared_state_cpu.py takes the objects
from the built library (nm, the writable data and bss symbols) and requires every one to match exactly one entry below,
so a new global cannot arrive unnoticed; DESIGN.md, "What the contexts of a process share", is the same list in prose.

SHARED: (pattern of the demangled name, guard, what it is, which test of tests/test_gpu_concurrent_contexts.py - or the CPU
program - reaches it from several threads). The guard starts with one of GUARDS.
TOOLCHAIN: objects the compiler, the linker or the HIP registration code make, each with the reason why no context's
thread writes it."""
import re
import subprocess

GUARDS = ("mutex ", "atomic", "thread_local", "one-time initialisation", "written only before any context exists")

SHARED = [
    # the device pool (devpool.cpp): one for all contexts of the process
    (r"flo::\(anonymous namespace\)::g_mu", "mutex g_mu", "the pool's mutex itself",
     "every test; tests/test_devpool_threads_cpu.py under ThreadSanitizer"),
    (r"flo::\(anonymous namespace\)::g_(live|free|cached)", "mutex g_mu", "the pool's maps of blocks out and cached, and the cached bytes",
     "every test; tests/test_devpool_threads_cpu.py under ThreadSanitizer"),
    (r"flo::g_pool_fill", "atomic", "flo_debug_pool_fill's setting", "different scenarios side by side (set while no thread runs)"),
    # the stream delay (stream_delay.hip)
    (r"flo::g_stream_delay", "atomic", "flo_debug_stream_delay's setting", "read by every launch of every pass"),
    (r"flo::g_stream_delays", "atomic", "the count of delays queued", "tests/test_gpu_late_streams.py (one thread)"),
    (r"_ZZN3floL10shader_mhzEvE3mhz(\.\d+)?|flo::shader_mhz\(\)::mhz", "atomic",
     "the shader clock read once (two threads may both read it from the driver and store the same value)", "tests/test_gpu_late_streams.py (one thread)"),
    # the file CRC's tables (container_kernels.hip)
    (r"flo::crc_mu", "mutex crc_mu", "the mutex of the CRC tables", "first use, raced: one-shot lossy encodes"),
    (r"flo::crc_(pow2|stripep|host_tables|dev_tables)", "mutex crc_mu", "host CRC tables made once, the device table once per device",
     "first use, raced: one-shot lossy encodes"),
    # "set the dynamic-LDS attribute once per (device, kernel)"
    (r"flo::allow_big_lds\(void const\*\)::(mu|done)", "mutex allow_big_lds()::mu", "the lossy kernels' attribute set",
     "first use, raced: one-shot lossy encodes"),
    (r"flo::rs_allow_lds\(void const\*\)::(mu|done)", "mutex rs_allow_lds()::mu", "the resample kernels' attribute set",
     "first use, raced: stage calls and resample"),
    (r"flo::np_allow_lds\(void const\*\)::(mu|done)", "mutex np_allow_lds()::mu", "the normalise kernels' attribute set",
     "first use, raced: normalise and true peaks"),
    # function-local statics with a constant initialiser
    (r"analysis_twiddles\(\)::tw_table", "one-time initialisation", "the analysis FFT's twiddles (const afterwards)", "first use, raced: analysis"),
    (r"\(anonymous namespace\)::term_table\(\)::t", "one-time initialisation", "the similarity score's term table (const afterwards)",
     "same scenario on every context: fingerprint index"),
    (r"encode_one\(.*\)::trace", "one-time initialisation", "whether FLO_TRACE was set at the first one-shot encode (const afterwards)",
     "first use, raced: one-shot lossy encodes"),
    (r"flo::stager_upload\(.*\)::small_limit", "one-time initialisation", "the upload size below which no ring is used (const afterwards)",
     "same scenario on every context: the batches; set to 0 in a child process of its own by "
     "tests/test_gpu_upload_paths.py::test_every_upload_through_the_ring_in_a_fresh_process"),
    (r"flo::upload_direct\(.*\)::two", "one-time initialisation", "whether large uploads use two copy threads (const afterwards)",
     "tests/test_gpu_late_streams.py::test_upload_encode_fetch_rounds (one thread); set in a child process of its own by "
     "tests/test_gpu_upload_paths.py::test_the_split_upload_in_a_fresh_process, and in the second run of "
     "tests/test_stager_paths_cpu.py"),
    # per thread
    (r"g_create_err(\[abi:cxx11\])?", "thread_local", "flo_ctx_create's error text", "error text stays with its owner"),
]

# Not in the library's writable data, so not listed: container.cpp's host_crc32()::tbl, a function-local static the issue of
# these tests names among the first-use sites. Its initialiser is a constant expression to the compiler, which folds the
# table into read-only data: there is no guard variable and nothing is written at run time (nm shows no such symbol of type
# b, B, d or D). Were it to become writable again, it would turn up here as an unlisted object.

TOOLCHAIN = [
    (r"guard variable for .*", "the guard of a function-local static: C++ one-time initialisation, by the compiler's runtime"),
    (r"__tls_guard", "the guard of this thread's thread_local initialisation: itself thread-local"),
    (r".*_kernel(<.*>)?\(.*\)", "a kernel's host-side handle: filled in by the loader's relocations, only its address is used"),
    (r"__hip_(fatbin_wrapper|gpubin_handle_[0-9a-f]+|cuid_[0-9a-f]+)", "the fat binaries' registration: written when the library is loaded"),
    (r"__do_(init|fini)\.__(initialized|finalized|object)", "the constructor's own once-flags: written when the library is loaded and unloaded"),
    (r"__dso_handle|_DYNAMIC|_GLOBAL_OFFSET_TABLE_|__init|__fini|__bss_start|_edata|_end|completed\.\d+|__TMC_END__",
     "made by the linker and the C runtime: written by the loader only"),
    (r"DW\.ref\..*|(typeinfo|vtable|typeinfo name) for .*", "language support data: relocated by the loader, constant afterwards"),
]


def writable_statics(lib_path):
    """the demangled names of the library's defined symbols in writable data and bss (nm types b, B, d, D), duplicates kept once"""
    out = subprocess.run(["nm", "-C", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    names = []
    for line in out.splitlines():
        m = re.match(r"^[0-9a-fA-F]*\s+([bBdD])\s+(.*)$", line)
        if m and m.group(2) not in names:
            names.append(m.group(2))
    return names


def classify(name):
    """-> ("shared", entry) | ("toolchain", entry) | (None, None), and how many entries matched"""
    hits = [("shared", e) for e in SHARED if re.fullmatch(e[0], name)] + [("toolchain", e) for e in TOOLCHAIN if re.fullmatch(e[0], name)]
    return (hits[0] if hits else (None, None)), len(hits)
