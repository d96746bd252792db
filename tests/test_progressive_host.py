"""Progressive rendering without a GPU: the schedule rtu_begin_render_progressive refuses before it creates a context, the new symbols in
the dynamic symbol tables of both libraries (read from the ELF files, HIP is not initialised), and the ctypes signatures of the binding."""
import ctypes
import os
import struct

import pytest

from conftest import GOLDEN

HIP_NEW = ["rtu_progressive_begin", "rtu_progressive_advance", "rtu_progressive_status", "rtu_progressive_snapshot_device",
           "rtu_progressive_snapshot", "rtu_progressive_free"]
HOST_NEW = ["rtu_begin_render_progressive"]


def dynamic_symbols(path):
    """Names of the defined symbols of an ELF64 little-endian shared object's .dynsym."""
    data = open(path, "rb").read()
    assert data[:4] == b"\x7fELF" and data[4] == 2 and data[5] == 1, "not an ELF64 little-endian file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for sh in sections:
        if sh[1] != 11:  # SHT_DYNSYM
            continue
        strtab = sections[sh[6]]
        for off in range(sh[4], sh[4] + sh[5], sh[9]):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", data, off)
            if st_shndx == 0:  # undefined here
                continue
            end = data.index(b"\0", strtab[4] + st_name)
            names.add(data[strtab[4] + st_name:end].decode())
    return names


@pytest.mark.parametrize("lib,names", [("librtu_hip.so", HIP_NEW), ("librtu_host.so", HOST_NEW)])
def test_new_symbols_are_exported(pkg, lib, names):
    syms = dynamic_symbols(os.path.join(os.path.dirname(pkg.__file__), "lib", lib))
    missing = [n for n in names if n not in syms]
    assert not missing, "%s does not export %s" % (lib, missing)
    assert set(names) <= set(pkg.HIP_SYMBOLS if lib == "librtu_hip.so" else pkg.HOST_SYMBOLS)


def test_binding_signatures(pkg):
    P, I = ctypes.c_void_p, ctypes.c_int
    assert pkg.RTU_ERR_STALE == -10
    hip, host = pkg.hip, pkg.host
    assert hip.rtu_progressive_begin.restype is P
    assert hip.rtu_progressive_begin.argtypes == [P, ctypes.POINTER(pkg.RtuFrameDesc), ctypes.POINTER(pkg.RtuAdaptiveDesc), ctypes.POINTER(I)]
    assert hip.rtu_progressive_advance.argtypes == [P, I, P] and hip.rtu_progressive_advance.restype is I
    assert hip.rtu_progressive_status.argtypes == [P, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)]
    assert hip.rtu_progressive_snapshot_device.argtypes == [P, P, P, P]
    assert hip.rtu_progressive_snapshot.argtypes == [P, P, P]
    assert hip.rtu_progressive_free.argtypes == [P] and hip.rtu_progressive_free.restype is None
    f = host.rtu_begin_render_progressive
    assert f.restype is P
    assert f.argtypes == [P, P, ctypes.POINTER(I), I, I, I, ctypes.POINTER(pkg.RtuAdaptiveDesc), ctypes.POINTER(I), I, pkg.PASS_DONE, P,
                          ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    for name in ("advance", "status", "snapshot", "close"):
        assert callable(getattr(pkg.Progressive, name))
    assert callable(pkg.Context.progressive)


@pytest.mark.parametrize("case", ["short", "long", "zero_pass", "negative_pass", "no_pass", "adaptive_over_255", "gather_2", "no_samples"])
def test_bad_schedule_is_refused_before_any_context(pkg, case):
    """NULL and a message, at once: nothing is started, so no GPU is touched (these run on machines without one)."""
    scene = pkg.Scene.from_blob_file(os.path.join(GOLDEN, "p10_s4_160x120", "scene.rtus.gz"))
    img = pkg.Image(16, 16)
    devs = (ctypes.c_int * 1)(0)
    samples, gather, ad, passes = 8, 0, None, [1, 1, 2, 4]
    if case == "short":
        passes = [1, 1, 2, 3]
    elif case == "long":
        passes = [1, 1, 2, 4, 1]
    elif case == "zero_pass":
        passes = [1, 0, 3, 4]
    elif case == "negative_pass":
        passes = [4, -1, 5]
    elif case == "no_pass":
        passes = []
    elif case == "adaptive_over_255":
        samples, passes, ad = 300, [300], pkg.RtuAdaptiveDesc(8, 1, 0.005, 0)
    elif case == "gather_2":
        gather = 2
    elif case == "no_samples":
        samples, passes = 0, None
    sched = (ctypes.c_int * max(len(passes), 1))(*passes) if passes is not None else None
    job = pkg.host.rtu_begin_render_progressive(scene._h, img._h, devs, 1, samples, gather, ctypes.byref(ad) if ad is not None else None, sched,
                                                len(passes) if passes is not None else 0, pkg.PASS_DONE(), None, None, None, None)
    assert not job
    msg = pkg.host.rtu_host_last_error().decode()
    assert "rtu_begin_render_progressive" in msg, msg
    with pytest.raises(pkg.RtuError):
        pkg.ProgressiveJob(scene, img, [0], samples, gather, ad, passes)
    img.close()
    scene.close()
