"""The host side of the sharded best-sample spawn, without a GPU: the owner arithmetic the library parts its taps by
(sharding.owner_of_row) against the bands themselves (sharding.shard_rows), and the two entry points in the ctypes table."""
import ctypes as C

import pytest


def test_owner_of_row_agrees_with_shard_rows():
    from tendrils_amd import sharding
    for height in range(1, 131):
        for world in range(1, 9):
            owners = [None] * height
            for rank in range(world):
                row0, rows = sharding.shard_rows(height, world, rank)
                for row in range(row0, row0 + rows):
                    assert owners[row] is None
                    owners[row] = rank
            assert owners == [sharding.owner_of_row(height, world, row) for row in range(height)], (height, world)
    with pytest.raises(ValueError):
        sharding.owner_of_row(10, 3, 10)


def test_the_binding_holds_the_two_entry_points():
    from tendrils_amd import _capi
    ctx = C.c_void_p
    assert _capi.PROTOTYPES["th_spawn_sample_sharded"] == (C.c_int32, [ctx, C.POINTER(_capi.SpawnSampleUniforms), C.c_int32, C.c_int32])
    assert _capi.PROTOTYPES["th_spawn_sample_sharded"] == _capi.PROTOTYPES["th_spawn_sample"]
    assert _capi.PROTOTYPES["th_spawn_query"] == (C.c_int32, [ctx, C.POINTER(_capi.SpawnInfo)])
    # th_spawn_info: four u64 and two i32
    assert [(name, C.sizeof(kind)) for name, kind in _capi.SpawnInfo._fields_] == [
        ("taps", 8), ("local_taps", 8), ("sent_bytes", 8), ("received_bytes", 8), ("chunks", 4), ("reserved", 4)]
    assert C.sizeof(_capi.SpawnInfo) == 40


def test_the_hosts_name_the_chunk_option_alike():
    from tendrils_amd.particles import Particles
    assert Particles.OPTIONS["spawn_chunk_rows"] == 12
