"""Shape lists and TiledPlan variants of the fp32 tiled-family cases, shared by
tests/test_conv_routes_gpu.py (which runs them) and scripts/conv_plan_table.py
(which records their plans)."""


def _halo_variants():
    return [dict(halo_f32=True, halo_f32_wide=True, halo_f32_bm=64, halo_f32_ch=16),
            dict(halo_f32=True, halo_f32_wide=True, halo_f32_bm=128, halo_f32_ch=16),
            dict(halo_f32=True, halo_f32_wide=False, halo_f32_bm=64, halo_f32_ch=32),
            dict(halo_f32=True, halo_f32_wide=False, halo_f32_bm=128, halo_f32_ch=32),
            dict(halo_f32=True, halo_f32_wide=False, halo_f32_bm=64, halo_f32_ch=16),
            dict(halo_f32=True, halo_f32_wide=False, halo_f32_bm=128, halo_f32_ch=16),
            dict(halo_f32=True, halo_f32_wide=False, halo_f32_bm=0, halo_f32_ch=16),
            dict(halo_f32=True, halo_f32_wide=False, halo_f32_bm=64, halo_f32_ch=16, halo_f32_small=True),
            dict(halo_f32=False, halo_f32_wide=False, halo_f32_bm=64, halo_f32_ch=32)]


FP32_SHAPES = [  # N, H, W, C, K, R, stride, pad, relu, bias
    (4, 9, 7, 5, 6, 3, 1, 1, True, True), (4, 12, 12, 8, 16, 3, 2, 1, False, False),
    (2, 16, 16, 3, 64, 7, 2, 3, False, False), (3, 20, 18, 3, 64, 7, 2, 3, True, True),
    (2, 15, 15, 5, 72, 5, 1, 2, False, False), (3, 8, 8, 16, 32, 1, 2, 0, False, False),
    (5, 1, 1, 40, 70, 1, 1, 0, True, True), (4, 32, 32, 3, 6, 5, 1, 0, True, True),
    (4, 14, 14, 6, 16, 5, 1, 0, True, True), (3, 10, 11, 4, 8, 3, 1, 1, True, False),
    (2, 14, 14, 64, 64, 3, 1, 1, False, False), (2, 14, 14, 64, 128, 3, 2, 1, False, False),
    (2, 13, 13, 64, 128, 1, 2, 0, False, False), (3, 7, 7, 256, 96, 3, 1, 1, True, True),
    (2, 9, 9, 32, 36, 5, 2, 2, False, True), (8, 1, 1, 512, 12, 1, 1, 0, False, True),
    (10, 56, 56, 64, 64, 3, 1, 1, False, False)]
HALO_SHAPES = [(8, 56, 56, 64, 64), (2, 56, 56, 64, 64), (4, 14, 14, 256, 256), (4, 28, 28, 128, 128),
               (3, 7, 7, 512, 512), (2, 13, 9, 32, 64)]
XCD_SHAPES = [(8, 56, 64, 64, 3, 1, 1), (4, 28, 64, 128, 3, 2, 1), (4, 28, 64, 128, 1, 2, 0),
              (2, 40, 3, 64, 7, 2, 3)]
S2_SHAPES = [(4, 56, 64, 128), (2, 28, 128, 256), (3, 14, 256, 512), (2, 10, 64, 32)]
XCD_VARIANTS = [dict(wg_xcd=True, wg_bk16=False, wg_bk16_64=False),
                dict(wg_xcd=False, wg_bk16=False, wg_bk16_64=False),
                dict(wg_xcd=False, wg_bk16=True, wg_bk16_64=True)]

S2_VARIANTS = [dict(halo_f32_s2=True), dict(halo_f32_s2=False)]
