"""The two developer entry points tests/test_gpu_ieee_div.py drives (rplgpu_debug_force_ieee_div,
rplgpu_debug_validate_div): present in the built library, outside the public ABI, and refusing a NULL handle
before they touch the device."""
import ctypes as C

from rplidar_ros2_driver_amd import abi


def test_debug_divide_entry_points_exist_and_reject_null():
    lib = abi.load_library()
    force, validate = lib.rplgpu_debug_force_ieee_div, lib.rplgpu_debug_validate_div
    force.argtypes = [C.c_void_p, C.c_uint32]
    validate.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    force.restype = validate.restype = C.c_int32
    assert "rplgpu_debug_force_ieee_div" not in abi.ABI_SYMBOLS and "rplgpu_debug_validate_div" not in abi.ABI_SYMBOLS
    for mask in (0, 7, 8):
        assert force(None, mask) == abi.ERR_INVALID_ARG
    n = C.c_uint32(5)
    assert validate(None, 0.05, 20.0, 127, 127, C.byref(n)) == abi.ERR_INVALID_ARG
    assert validate(None, 0.05, 20.0, 127, 127, None) == abi.ERR_INVALID_ARG
    assert n.value == 5
