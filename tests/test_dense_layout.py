"""The one layout of several arrays in one buffer (engine_dense.aligned_offsets) that every upload and every ring slot uses."""


def test_aligned_offsets_against_offsets_written_out_by_hand():
    """every array starts at a multiple of 16 bytes; an empty array takes no room; sizes that are no multiple of 4 or 16 are rounded up"""
    from drecpy_amd.engine_dense import aligned_offsets
    assert aligned_offsets((1, 4, 5, 0, 3)) == ([0, 16, 32, 48, 48], 64)                    # bytes
    assert aligned_offsets([4 * n for n in (1, 4, 5, 0, 3)]) == ([0, 16, 32, 64, 64], 80)   # the same counts of int32: 4, 16, 20, 0, 12 bytes
    assert aligned_offsets(()) == ([], 0)
    assert aligned_offsets((16, 17)) == ([0, 16], 48)


def test_the_dmf_batch_layout_is_the_recorded_one():
    """DmfEngine._batch_layout(7): the tuple it returned before it became a caller of aligned_offsets"""
    from drecpy_amd.engine_dmf import DmfEngine
    assert DmfEngine._batch_layout(7) == ([0, 32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 16800],
                                          (7, 7, 7, 8, 8, 7, 7, 8, 8, 7, 7, 4110, 14), 16864)
    assert len(DmfEngine._BATCH_ARRAYS) == 13
