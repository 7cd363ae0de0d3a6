"""CPU: KeyframeStore.GROUPS, the one table the views, reads, writes and fills of the store's four groups of arrays
are driven by, names what the ctypes host structs have -- every column and every count is a field, and no pointer of
the geometry, life and appearance structs is left out.  No device and no library call."""
import ctypes

import pytest

from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import KeyframeStore

GROUPS = KeyframeStore.GROUPS


def pointer_fields(T):
    return {f for f, t in T._fields_ if t is ctypes.c_void_p}


def test_the_four_groups():
    assert list(GROUPS) == ["main", "geometry", "life", "appearance"]


@pytest.mark.parametrize("group", list(GROUPS))
def test_columns_and_counts_are_fields_of_the_host_struct(group):
    g = GROUPS[group]
    fields = {f for f, _ in g["host"]._fields_}
    assert g["cols"], group
    for k, (dtype, width, count, plus) in g["cols"].items():
        assert k in pointer_fields(g["host"]), (group, k)
        assert count in fields or count in KeyframeStore.COUNTS, (group, k, count)
        assert width >= 1 and plus in (0, 1), (group, k)


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_pointer_of_the_host_struct_is_a_column(group):
    assert set(GROUPS[group]["cols"]) == pointer_fields(GROUPS[group]["host"]), group


def test_the_groups_cover_the_geometry_life_and_appearance_structs():
    named = set().union(*(g["cols"] for g in GROUPS.values()))
    for T in (A.KfStoreGeomHost, A.KfStoreLifeHost, A.KfStoreAppearHost):
        assert pointer_fields(T) <= named, (T.__name__, pointer_fields(T) - named)


def test_entry_points_are_named_for_what_a_group_can_do():
    for group, g in GROUPS.items():
        assert g["view"][0].startswith("lorb_kf_store_") and g["read"].startswith("lorb_kf_store_"), group
        assert ("write" in g) == ("fault" in g), group   # a group that can be written states its length message
