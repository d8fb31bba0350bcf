"""Host only: the case table of tests/_strided_cases.py covers every form of the LDS slab kernel (csrc/bfp_slab.hip) that its
launcher can select, by the restatement of the launcher's rules in the same module.  The GPU tests
(tests/test_gpu_strided_blocks.py) hold the restatement against the library: accepted <=> the internal entry returns 0."""
import _strided_cases as S


def test_the_table_covers_every_form_of_the_slab_kernel():
    forms = S.forms_of(S.SLAB_TABLE)
    missing = [f for f in S.REQUIRED_FORMS if f not in forms]
    assert not missing, missing
    # dtype x precision x symmetry: every case of the table runs DTYPE_NAMES x VARIANTS, which must hold both sides of each switch
    assert set(S.DTYPE_NAMES) == {"bf16", "f16"}
    for dt in S.DTYPE_NAMES:
        for single in (True, False):
            for sym in (True, False):
                assert any(S.single_rounding_ok(dt, wl) == single and s == sym for wl, s in S.VARIANTS), (dt, single, sym)


def test_removing_a_form_from_the_table_is_noticed():
    """the coverage assertion is not vacuous: without its only case, each required form goes missing"""
    for f in S.REQUIRED_FORMS:
        holders = [c for c in S.SLAB_TABLE if f in S.forms_of([c])]
        assert holders, f
        rest = [c for c in S.SLAB_TABLE if c not in holders]
        assert f not in S.forms_of(rest), f


def test_restated_geometry_of_the_shapes_the_kernel_was_sized_for():
    """figures stated in csrc/bfp_slab.hip's header and launcher comments, recomputed"""
    g = S.slab_geometry(64, 512, 28 * 28, 64)
    assert g.accepted and (g.lds, g.lanes, g.per, g.Q, g.NV, g.tiles, g.pitch % 32) == (98 * S.KIB, 1024, 16, 4, 8, 512, 8)
    g = S.slab_geometry(256, 1024, 14 * 14, 64)
    assert g.accepted and (g.lanes, g.tiles, g.NV) == (256, 4096, 8)
    g = S.slab_geometry(8 * 32, 2048, 128, 64)
    assert g.accepted and g.lds == 16 * S.KIB + 64 * 8 * 4 and not S.slab_preferred(128, 64)      # whole-line rows: column kernel
    assert not S.slab_geometry(1, 512, 18 * 18, 256).accepted and not S.slab_geometry(64, 256, 56 * 56, 64).accepted
    assert S.slab_geometry(2, 3, 224 * 224, 64).reason == "slab over 150 KiB"
    for c in S.SLAB_TABLE:
        o, L, inner, g = S.case_geometry(c)
        assert g.accepted == (not c.name.startswith("r_")), (c.name, g.reason)
        if g.accepted:
            assert g.lanes == int(c.name.split("_")[0][1:]) and g.lds <= 150 * S.KIB and g.pitch * 2 >= inner and g.NV * g.lanes * 8 >= g.B * inner
            assert g.per * g.Q == g.B and (g.Q == 1 or g.pitch % 32 == 32 // g.Q), c.name


def test_loop_sizes_reach_a_second_and_third_trip():
    """the sizes the persistent-loop tests derive give every workgroup at least two tiles and some three, whatever the CU count"""
    for cus in (2, 3, 64, 256, 304):
        for c in S.SLAB_TABLE:
            g = S.case_geometry(c)[3]
            if not g.accepted or g.lanes != 1024:
                continue
            gm = S.slab_grid_max(cus, g.lds)
            outer = S.outer_for(c, -(-5 * gm // 2), gm)
            tiles = outer * g.nblk
            assert tiles * 2 >= 5 * gm and (tiles % gm != 0 or g.nblk % gm == 0) and S.case_geometry(c, outer)[3].accepted, (cus, c.name)
    assert S.slab_grid_max(256, 98 * S.KIB) == 256 and S.outer_for(S.SLAB_BY_NAME["s1024_per16"], 640, 256) == 80   # [80,512,28,28]: 640 tiles
