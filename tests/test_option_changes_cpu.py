"""The CPU oracle, run segment by segment with its states carried, reproduces the reference's encode() closures under option
changes between frames (tests/golden/option_changes.json).  This pins the model the GPU tests compare the stream against."""
import pytest

import option_changes_lib as OC

FIX = OC.fixture()
CASES = [(name, sig) for name, s in FIX['schedules'].items() for sig in s['results']]


@pytest.mark.parametrize('name,sig', CASES, ids=['%s-%s' % c for c in CASES])
def test_oracle_reproduces_reference_schedule(name, sig):
    s = FIX['schedules'][name]
    frames = FIX['frames']
    chans = OC.signal(FIX['signals'][sig], frames)
    units = OC.oracle_encode(chans, OC.options_at(s['initial'], s['changes'], frames))
    err = OC.check_against(s['results'][sig], units, len(chans))
    assert err is None, err


def test_fixture_covers_the_switch_that_needs_kept_history():
    """detection -> fixed -> detection: the first detected frame is compared with the last detected one, not its neighbour"""
    s = FIX['schedules']['detect_223_detect']
    assert [f for f, _ in s['changes']] == [16, 40]
    per_frame = OC.options_at(s['initial'], s['changes'], FIX['frames'])
    assert per_frame[39]['fixedBlockModes'] == [2, 2, 3] and per_frame[40]['fixedBlockModes'] is None


def test_fixture_tables_are_committed():
    """every bias of the schedules has a committed pow table, so the oracle runs on the reference's own numbers"""
    tables = OC.O.golden_tables()['biased_scale_factors_f64']
    for s in FIX['schedules'].values():
        for v in OC.options_at(s['initial'], s['changes'], FIX['frames']):
            b = v['allocationBias']
            assert b == 1 or any(float(k) == b for k in tables), b
