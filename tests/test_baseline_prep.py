"""Host side of cvig_baseline's packed data path (witw_amd/baseline_data.py, csrc/baseline_prep.hip): the roll start against
horizontal_shift, the argument checks of the two C entries (no launch, no GPU), the packed collate of an empty share."""
import pytest
import torch


@pytest.mark.parametrize('W', [360, 1232, 53])
def test_roll_start_is_horizontal_shifts_roll(W):
    from witw_amd import baseline_data as bd
    from witw_amd import cvig_baseline as cb
    img = torch.arange(W, dtype=torch.float32).reshape(1, 1, W).repeat(3, 2, 1)
    angles = [0., 360, 360., 719.9, 33.3, 301.0, -17.5, -359.9, -360., 180., 90]
    for cols in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, W - 0.5, W / 2 + 0.5):      # exact .5 columns at W = 360; the neighbourhood of one elsewhere
        angles.append(cols * 360. / W)
    for a in angles:
        want = cb.horizontal_shift(img, a, unit='degrees')
        start = bd.roll_start(a, W)
        assert isinstance(start, int) and 0 <= start < W, (a, start)
        assert torch.equal(want, torch.roll(img, -start, -1)), (W, a, start)
        assert int(want[0, 0, 0]) == start, (W, a, start)          # the left roll: column `start` arrives at column 0
    if W == 360:      # half-to-even, as Python rounds: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
        assert [bd.roll_start(c, 360) for c in (0.5, 1.5, 2.5, -0.5, -1.5)] == [0, 2, 2, 0, 358]


def test_entries_refuse_bad_arguments_without_a_launch():
    from witw_amd import _lib
    lib = _lib.load()
    rot, roll = lib.witw_baseline_rotate_batched, lib.witw_baseline_roll_rows_batched

    def refused(rc, word):
        msg = lib.witw_last_error()
        assert rc < 0 and word in msg, (rc, msg)
        with pytest.raises(_lib.WitwError):
            _lib.check(rc, 'entry')

    # (desc, theta, y, B, C, H, W, kind, stream); 1 stands for a non-null pointer that is never dereferenced
    refused(rot(None, 1, 1, 2, 3, 8, 8, 1, None), b'null')
    refused(rot(1, None, 1, 2, 3, 8, 8, 1, None), b'null')
    refused(rot(1, 1, None, 2, 3, 8, 8, 1, None), b'null')
    refused(rot(1, 1, 1, 2, 3, 8, 8, 2, None), b'kind 2')
    refused(rot(1, 1, 1, 2, 0, 8, 8, 1, None), b'C=0')
    refused(rot(1, 1, 1, 2, 9, 8, 8, 0, None), b'C=9')
    refused(rot(1, 1, 1, 0, 3, 8, 8, 1, None), b'bad shape')
    refused(rot(1, 1, 1, 2, 3, 0, 8, 1, None), b'bad shape')
    refused(rot(1, 1, 1, 2, 3, 8, -1, 1, None), b'bad shape')
    # (desc, y, B, C, Ho, Wo, rep, kind, stream)
    refused(roll(None, 1, 2, 3, 8, 8, 2, 1, None), b'null')
    refused(roll(1, None, 2, 3, 8, 8, 2, 1, None), b'null')
    refused(roll(1, 1, 2, 3, 8, 8, 2, 2, None), b'kind 2')
    refused(roll(1, 1, 2, 0, 8, 8, 2, 1, None), b'C=0')
    refused(roll(1, 1, 2, 9, 8, 8, 2, 0, None), b'C=9')
    refused(roll(1, 1, 2, 3, 8, 8, 0, 1, None), b'rep=0')
    refused(roll(1, 1, 2, 3, 8, 8, -2, 1, None), b'rep=-2')
    refused(roll(1, 1, 2, 3, 7, 8, 2, 1, None), b'Ho=7')            # Ho != rep * H for any H
    refused(roll(1, 1, 2, 3, 0, 8, 1, 1, None), b'bad shape')
    refused(roll(1, 1, 0, 3, 8, 8, 1, 1, None), b'bad shape')


def test_wrappers_refuse_host_tables():
    from witw_amd import _lib
    from witw_amd import baseline_data as bd
    desc = torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(_lib.WitwError, match='GPU tensor'):
        bd.rotate_batched(desc, [0., 0.], 2, 3, (8, 8), kind=1)
    with pytest.raises(_lib.WitwError, match='GPU tensor'):
        bd.roll_rows_batched(desc, 2, 3, (8, 8), rep=1, kind=1)


def test_packed_collate_of_an_empty_share_is_the_raw_empty_batch():
    from witw_amd import cvig_baseline as cb
    from witw_amd import cvig_fov
    assert cb.collate_packed([]) == {'surface': [], 'overhead': []} == cvig_fov.collate_raw([])
    assert cb.collate_packed([], ring=object()) == {'surface': [], 'overhead': []}      # before a ring slot is taken
    with pytest.raises(_lib_error()):
        cb.train(data_path='zip')
    with pytest.raises(_lib_error()):
        cb.test(data_path='zip')
    assert cb.Globals.data_path == 'reference'


def _lib_error():
    from witw_amd import _lib
    return _lib.WitwError
