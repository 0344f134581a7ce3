"""ctypes binding of libr3dg_hip.so; every signature is read from include/r3dg_hip.h itself (_abi.py).  There is NO fallback: if
the HIP library is missing or a call fails, the op raises -- a silent CPU/eager path would void every parity claim."""
import ctypes as C
import threading
import os

from . import _abi
from ._abi import ALLOC_FN  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# R3DG_LIB_PATH: an experiment build of the SAME library (tools/build_variant.py) for A/B measurements; never a fallback
LIB_PATH = os.environ.get("R3DG_LIB_PATH") or os.path.join(_HERE, "lib", "libr3dg_hip.so")

_lib = None


def lib():
    """Load the HIP library (once).  Raises RuntimeError with build instructions if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libr3dg_hip.so not found at %s -- build it with `python -m relightable3dgaussian_amd.build` "
                "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
        # PyTorch-ROCm ships its own HIP runtime; it must be in the process BEFORE this library is loaded so that both
        # resolve to ONE runtime instance (loaded the other way round, the library's kernels see "no ROCm-capable
        # device" once torch has initialised its copy)
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _abi.prototypes.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


OPTIONS = _abi.options       # enum r3dg_option, by index


def set_option(name, value):
    """r3dg_set_option by name (experiments / tests): set_option("CULL", 0)."""
    check(lib().r3dg_set_option(OPTIONS.index(name), int(value)), "set_option(%s)" % name)


_live_lock = threading.Lock()
_live_entries = {}          # context handle -> number of `with` blocks (any thread) currently inside it


class OptionContext:
    """Tuning options that belong to ONE object (include/r3dg_hip.h "option contexts"): `ctx.set("RESERVE_CUS", 8)`, then
    `with ctx:` around the object's library calls -- inside, launches of the calling thread see the context's values where it
    sets them and the process defaults elsewhere; the previous context is restored on exit (contexts nest)."""

    def __init__(self, **options):
        self._h = lib().r3dg_context_create()
        if self._h is None:                      # (NULL)
            raise RuntimeError("r3dg_context_create failed")
        # the restore stack is PER THREAD, like the library's "current context": two threads inside the same object's context
        # (a worker polling while the main thread is in an iteration) must not pop each other's saved handles
        self._tls = threading.local()
        for k, v in options.items():
            self.set(k, v)

    def set(self, name, value):
        check(lib().r3dg_context_set_option(self._h, OPTIONS.index(name), int(value)), "context_set_option(%s)" % name)

    def __enter__(self):
        prev = C.c_void_p()
        check(lib().r3dg_context_make_current(self._h, C.byref(prev)), "context_make_current")
        stack = getattr(self._tls, "prev", None)
        if stack is None:
            stack = self._tls.prev = []
        stack.append(prev.value)
        with _live_lock:
            _live_entries[self._h] = _live_entries.get(self._h, 0) + 1
        return self

    def __exit__(self, *exc):
        check(lib().r3dg_context_make_current(self._tls.prev.pop(), None), "context_make_current")
        with _live_lock:
            n = _live_entries.get(self._h, 0) - 1
            if n > 0:
                _live_entries[self._h] = n
            else:
                _live_entries.pop(self._h, None)
        return False

    def __del__(self):
        # (a context that some thread is still inside -- current there, or saved as another context's "previous" -- is leaked
        # rather than destroyed: the library would dereference the freed handle at that thread's next launch)
        try:
            if self._h:
                with _live_lock:
                    busy = _live_entries.get(self._h, 0) > 0
                if not busy:
                    lib().r3dg_context_destroy(self._h)
                self._h = None
        except Exception:
            pass


def get_option(name):
    v = C.c_int(0)
    check(lib().r3dg_get_option(OPTIONS.index(name), C.byref(v)), "get_option(%s)" % name)
    return v.value


def check(status, what):
    if status != 0:
        msg = lib().r3dg_last_error()
        raise RuntimeError("%s failed (%d): %s" % (what, status, msg.decode() if msg else "?"))


def ptr(t):
    """Device pointer of a torch tensor, or None for an absent optional (numel()==0: the reference passes empty
    CPU tensors for absent optionals, gaussian_renderer/r3dg_rasterization.py:235-245)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def current_stream():
    """The raw HIP stream torch launches on right now (of the current device).  torch.cuda.current_stream() builds a Stream
    object through half a dozen Python layers (10 us; the fused iteration asks 16 times): the C accessor it ends in is used
    directly when this torch has it."""
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return raw(torch._C._cuda_getDevice())
    return torch.cuda.current_stream().cuda_stream


def stream_wait(waiter, signaller):
    """`waiter` (a torch.cuda.Stream) waits for everything queued on `signaller` so far: torch's waiter.wait_stream(signaller)
    through the library's pooled events (r3dg_stream_wait_stream)."""
    check(lib().r3dg_stream_wait_stream(waiter.cuda_stream, signaller.cuda_stream), "stream_wait_stream")


def shader_clock_ghz(device="cuda", iters=4000):
    """The shader clock under VALU load, measured on the device itself (r3dg_clock_probe): cycles of the shader-clock counter per
    tick of the constant-rate wall clock, summed over a device-filling grid of FMA-only waves.  -> (GHz, waves that reported)."""
    import torch
    out = torch.zeros(3, dtype=torch.int64, device=device)
    sink = torch.zeros(1, dtype=torch.float32, device=device)
    khz = C.c_int(0)
    with torch.cuda.device(out.device):
        check(lib().r3dg_clock_probe(current_stream(), int(iters), out.data_ptr(), sink.data_ptr(), C.byref(khz)), "clock_probe")
        torch.cuda.synchronize()
    cyc, ticks, waves = (int(v) for v in out.tolist())
    return (cyc / max(ticks, 1)) * khz.value * 1e-6, waves


def profile_read():
    """{stage name: (total ms, launches)} since the last r3dg_profile_enable(1)."""
    L = lib()
    n = L.r3dg_profile_num_stages()
    ms = (C.c_double * n)()
    cnt = (C.c_int * n)()
    check(L.r3dg_profile_read(ms, cnt), "profile_read")
    return {L.r3dg_profile_stage_name(i).decode(): (ms[i], cnt[i]) for i in range(n)}
