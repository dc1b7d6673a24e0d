"""The layout arithmetic under the device scratch of the resident-panel scans (snpmatch_amd/csrc/snpm_scratch.hpp), on the host."""
import host_kernel_util


def test_scratch_layout_under_sanitizers(tmp_path):
    """tests/scratch_host_driver.cpp under ASan + UBSan, each layout assigned on a block of exactly total() bytes and every byte of
    every part written: one part of one byte; parts of 4095 / 4096 / 4097 bytes in a row; a part of no elements between two others
    (a valid pointer that aliases nothing); twelve parts, and the thirteenth refused; a byte size, a rounded size and a running
    total past SIZE_MAX, each refused with nothing assigned; uint8 / int32 / double / uint64 pointers, each aligned to 4096"""
    cases = host_kernel_util.run_driver("scratch_host_driver", tmp_path)
    assert [ln.split()[1] for ln in cases] == ["one-byte", "page-edges", "zero-part", "twelve-parts", "thirteenth-refused", "overflow-bytes",
                                               "overflow-rounding", "overflow-total", "typed", "empty"]
