"""GPU tier of "one map, four block sizes": the cases of tests/block_size_case.py on the real device.  One voxel content is
uploaded at 8, 16, 32 and 64 voxels per side; the result of every reader at 8 is checked against the NumPy models (once, shared
by the four cases), and the results at the other sizes against it."""
import pytest

from tests import block_size_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(block_size_case.SPECS, key=lambda n: (block_size_case.SPECS[n].get("case", ""), block_size_case.SPECS[n]["vps"])))
def test_readers_do_not_depend_on_the_block_size(name):
    block_size_case.run_case(block_size_case.SPECS[name])


def test_upload_and_download_of_more_blocks_than_one_staging_chunk():
    """12 blocks of 64^3 voxels along x (-6 .. 5; a chunk holds 11): the second chunk's offsets, for both arrays, the tsdf alone,
    and the blocks in reversed order."""
    block_size_case.case_chunks(dict(vps=64, blocks=12))
