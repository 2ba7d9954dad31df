"""The recurrent-policy fixtures are the reference's archives' weights (oracle/check_lstm_fixtures.py):
every parameter of tests/golden/lstm_policy_<robot>.npz equals, byte for byte, the raw tensor storage
of deploy/pre_train/<robot>/motion.pt (read from the zip, nothing unpickled or executed), and the
memory states are those of the fixture's own 5-step post-reset run.  The archives' storages are
recorded as lengths and SHA-256 digests in tests/golden/lstm_archive_storages.json, so the check
runs wherever the repository does."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))


@pytest.mark.parametrize("robot", ["g1", "h1", "h1_2"])
def test_lstm_fixture_is_the_archive(robot):
    import check_lstm_fixtures as chk
    assert chk.check(None, robot) == []
