"""The default blocked plan's mapping (ops.BlockedPlan.resolve): request -> fine blocks and
row_edges.  No GPU and no libgta: the knob values are passed in."""
import pytest

from gta_graph_tensor_acclelrator_for_general_gnn_amd.ops import BlockedPlan

IE = BlockedPlan.ITEM_EDGES


@pytest.mark.parametrize("blocks,pct,want", [
    (20, 100, 20), (20, 120, 24), (20, 140, 28), (20, 160, 32), (20, 200, 40), (24, 160, 38),
    (16, 150, 24), (17, 150, 26),    # 25.5 rounds up
    (40, 160, 63), (63, 100, 63), (63, 200, 63), (32, 200, 63),  # the cap
])
def test_default_request_maps_to_fine_blocks(blocks, pct, want):
    assert BlockedPlan.resolve(blocks, knobs=(pct, 16, 16)) == (want, IE, 16)
    assert BlockedPlan.resolve(blocks, knobs=(pct, 0, 16)) == (want, IE, 0)


def test_requests_below_the_minimum_keep_their_blocks():
    for blocks in (1, 4, 10, 15):
        assert BlockedPlan.resolve(blocks, knobs=(160, 16, 16)) == (blocks, IE, BlockedPlan.ROW_EDGES)
    assert BlockedPlan.resolve(16, knobs=(160, 16, 16)) == (26, IE, 16)
    assert BlockedPlan.resolve(10, knobs=(160, 16, 1)) == (16, IE, 16)


@pytest.mark.parametrize("blocks", [1, 5, 20, 63])
def test_named_arguments_are_left_alone(blocks):
    knobs = (200, 32, 1)
    assert BlockedPlan.resolve(blocks, 128, None, knobs) == (blocks, 128, BlockedPlan.ROW_EDGES)
    assert BlockedPlan.resolve(blocks, None, 0, knobs) == (blocks, IE, 0)
    assert BlockedPlan.resolve(blocks, None, 24, knobs) == (blocks, IE, 24)
    assert BlockedPlan.resolve(blocks, 7, 40, knobs) == (blocks, 7, 40)
    assert BlockedPlan.resolve(blocks, IE, BlockedPlan.ROW_EDGES, knobs) == (blocks, IE, BlockedPlan.ROW_EDGES)


def test_inert_knobs_reproduce_the_request():
    for blocks in (16, 20, 24, 63):
        assert BlockedPlan.resolve(blocks, knobs=(100, 0, 16)) == (blocks, IE, 0)
