"""rocprofv3 kernel name -> in-library profiler label (ProfLabel, csrc/se_kernels.h): ONE table, read by bench.py's PMC
traffic pass and by tools/pmc_summary.py, so that every label the profiler prints has its HBM traffic beside it.
Keys are prefixes of the demangled kernel name with the `se::` namespace stripped; the first matching prefix wins, so
longer prefixes come first where one name is the prefix of another."""

KERNEL_LABELS = {
    # 96 -> 192 (N = 192 packed rows)
    "wino_kernel": "wino_n192", "wino24_kernel": "wino_n192", "rconv16": "gconv_n192", "gconv_kernel<12": "gconv_n192",
    # 48 -> 96 / 24 -> 96
    "wino48_kernel": "wino_n96", "rconv96": "gconv_n96", "gconv_kernel<6": "gconv_n96",
    # 48 -> 96 / 192 at stride 2 in 96-row halves (polyphase F(2,2), se_s2poly.hip)
    "s2poly48_kernel": "wino_n96",
    "winoup_kernel": "wino_up96",
    # 48 output rows: 5x5 heads, 24 -> 48 stride 2, gen_deconv 48 -> 48
    "winoup48_kernel": "gconv_n48", "rtile_dense5w_kernel": "gconv_n48", "rtile_dense5_kernel": "gconv_n48",
    "rtile_kernel<3": "gconv_n48", "gconv_kernel<3": "gconv_n48",
    # 24 -> 24 at full resolution
    "rtilew2_kernel": "gconv_n24", "rtilew_kernel": "gconv_n24", "rtile_kernel<2": "gconv_n24", "gconv_kernel<2": "gconv_n24",
    "dtail_kernel": "dtail",
    # attention
    "att2_pair_kernel": "att_score", "att2_pv_kernel": "att_pv",
    "att2_softmax": "att_softmax", "att2_stats": "att_softmax",
    "att2_boxsum": "att_boxsum", "att2_ptilde": "att_boxsum",
    "att2_prep": "att_prep", "att2_transpose": "att_prep", "att2_emean": "att_prep", "att2_eoff": "att_prep",
    "att2_similar": "layout",
    # the rest
    "small_conv_kernel": "small_conv", "pack_": "pack", "colreduce": "colreduce", "vecbias_kernel": "colreduce",
    "nchw_to_nhwc": "layout", "nhwc_to_nchw": "layout", "nhwc16_to_nchw": "layout", "quantize_u8_kernel": "layout",
    "dequant_u8_kernel": "layout",
    # the ends of a window edit at a working size (se_resize.hip; before the plain resize names: first matching prefix wins)
    "(anonymous namespace)::window_resample_h_kernel": "window_resample_h", "(anonymous namespace)::window_paste_v_kernel": "window_paste_v",
    "window_resample_h_kernel": "window_resample_h", "window_paste_v_kernel": "window_paste_v",
    # the demo's per-request resizes (se_resize.hip)
    "(anonymous namespace)::resample_h_kernel": "resize_h", "(anonymous namespace)::resample_v_kernel": "resize_v",
    "resample_h_kernel": "resize_h", "resample_v_kernel": "resize_v",
    # window edits of a resident frame (se_window.hip)
    "(anonymous namespace)::window_gather_kernel": "window_gather", "(anonymous namespace)::window_border_kernel": "window_border",
    "(anonymous namespace)::window_paste_kernel": "window_paste",
    "window_gather_kernel": "window_gather", "window_border_kernel": "window_border", "window_paste_kernel": "window_paste",
    # the feathered paste of a session (se_feather.hip)
    "(anonymous namespace)::window_paste_feather_kernel": "window_paste_feather", "window_paste_feather_kernel": "window_paste_feather",
    # fills of a painted region (se_fill.hip)
    "(anonymous namespace)::fill_masks_kernel": "fill_masks", "(anonymous namespace)::fill_keep_kernel": "fill_keep",
    "fill_masks_kernel": "fill_masks", "fill_keep_kernel": "fill_keep",
    # selection by colour (se_select.hip)
    "(anonymous namespace)::select_similar_kernel": "select_similar", "(anonymous namespace)::select_flood_kernel": "select_flood",
    "(anonymous namespace)::select_grow_kernel": "select_grow",
    "select_similar_kernel": "select_similar", "select_flood_kernel": "select_flood", "select_grow_kernel": "select_grow",
    # modify a selection's shape (se_modify.hip): expand / contract by a disc, and the majority vote in it
    "(anonymous namespace)::modify_disc_kernel": "modify_disc", "(anonymous namespace)::modify_vote_kernel": "modify_vote",
    "modify_disc_kernel": "modify_disc", "modify_vote_kernel": "modify_vote",
    # lasso selections and their algebra (se_lasso.hip)
    "(anonymous namespace)::lasso_fill_kernel": "lasso_fill", "(anonymous namespace)::plane_combine_kernel": "plane_combine",
    "lasso_fill_kernel": "lasso_fill", "plane_combine_kernel": "plane_combine",
    # the outline of a selection (se_outline.hip): one tile kernel in two forms, and the scan between them
    "(anonymous namespace)::outline_tile_kernel<false>": "outline_count", "(anonymous namespace)::outline_tile_kernel<true>": "outline_emit",
    "(anonymous namespace)::outline_scan_kernel": "outline_scan",
    "outline_tile_kernel<false>": "outline_count", "outline_tile_kernel<true>": "outline_emit", "outline_scan_kernel": "outline_scan",
    # move or clone a selection (se_move.hip): the drop without and with a soft edge, and the shift of the plane
    "(anonymous namespace)::move_drop_kernel<false>": "move_drop", "(anonymous namespace)::move_drop_kernel<true>": "move_drop",
    "(anonymous namespace)::plane_shift_kernel": "plane_shift",
    "move_drop_kernel<false>": "move_drop", "move_drop_kernel<true>": "move_drop", "plane_shift_kernel": "plane_shift",
    # seamless move and clone (se_blend.hip): the rim's classification, the pull, the sweeps of a level, the drop
    "(anonymous namespace)::blend_init_kernel": "blend_init", "(anonymous namespace)::blend_pull_kernel": "blend_pull",
    "(anonymous namespace)::blend_relax_kernel": "blend_relax", "(anonymous namespace)::blend_apply_kernel": "blend_apply",
    "blend_init_kernel": "blend_init", "blend_pull_kernel": "blend_pull", "blend_relax_kernel": "blend_relax",
    "blend_apply_kernel": "blend_apply",
    # the canvas of a session (se_canvas.hip): the walk of the output's bytes, and the quarter turn through the LDS
    "(anonymous namespace)::canvas_map_kernel": "canvas_map", "(anonymous namespace)::canvas_turn_kernel": "canvas_turn",
    "canvas_map_kernel": "canvas_map", "canvas_turn_kernel": "canvas_turn",
    # scale and rotate a selection (se_warp.hip): the resampling drop, and the warp of the plane
    "(anonymous namespace)::warp_drop_kernel": "warp_drop", "(anonymous namespace)::plane_warp_kernel": "plane_warp",
    "warp_drop_kernel": "warp_drop", "plane_warp_kernel": "plane_warp",
    # blur, sharpen or pixelate a selection (se_filter.hip): the separable filter by radius class, and the block mean
    "(anonymous namespace)::filter_blur_kernel<8>": "filter_blur", "(anonymous namespace)::filter_blur_kernel<16>": "filter_blur",
    "(anonymous namespace)::filter_blur_kernel<32>": "filter_blur", "(anonymous namespace)::filter_mosaic_kernel": "filter_mosaic",
    "filter_blur_kernel<8>": "filter_blur", "filter_blur_kernel<16>": "filter_blur", "filter_blur_kernel<32>": "filter_blur",
    "filter_mosaic_kernel": "filter_mosaic",
    # adjust a selection's tone and colour (se_adjust.hip): the pointwise kernel, the histogram's two steps, the table builder
    "(anonymous namespace)::adjust_kernel": "adjust", "(anonymous namespace)::hist_tiles_kernel": "hist_tiles",
    "(anonymous namespace)::hist_sum_kernel": "hist_sum", "(anonymous namespace)::adjust_lut_kernel": "adjust_lut",
    "adjust_kernel": "adjust", "hist_tiles_kernel": "hist_tiles", "hist_sum_kernel": "hist_sum", "adjust_lut_kernel": "adjust_lut",
    # the undo journal of a session (se_window.hip)
    "(anonymous namespace)::window_save_kernel": "window_save", "(anonymous namespace)::window_swap_kernel": "window_swap",
    "window_save_kernel": "window_save", "window_swap_kernel": "window_swap",
    # region edits: the tile pass over a full-size sketch (se_window.hip)
    "(anonymous namespace)::sketch_tiles_kernel": "sketch_tiles", "sketch_tiles_kernel": "sketch_tiles",
    # strokes as polylines: the rasteriser of the windows' sketches (se_window.hip)
    "(anonymous namespace)::sketch_strokes_kernel": "sketch_strokes", "sketch_strokes_kernel": "sketch_strokes",
    # the device PNG encoder of the editing sessions (se_png.hip)
    "(anonymous namespace)::png_rows_kernel": "png_rows", "(anonymous namespace)::png_stripe_kernel": "png_stripes",
    "(anonymous namespace)::png_finish_kernel": "png_finish",
    "png_rows_kernel": "png_rows", "png_stripe_kernel": "png_stripes", "png_finish_kernel": "png_finish",
    # the device JPEG encoder of the editing sessions (se_jpg.hip)
    "(anonymous namespace)::jpg_blocks_kernel": "jpg_blocks", "(anonymous namespace)::jpg_rows_kernel": "jpg_rows",
    "(anonymous namespace)::jpg_finish_kernel": "jpg_finish",
    "jpg_blocks_kernel": "jpg_blocks", "jpg_rows_kernel": "jpg_rows", "jpg_finish_kernel": "jpg_finish",
    # its kernels for 4:2:0 sampling and per-image Huffman tables (se_jpg.hip).  No kernel is named jpg2_rows_kernel any more (the one
    # row kernel is jpg_rows_kernel); the entries stay for the committed traces that name it
    "(anonymous namespace)::jpg2_blocks420_kernel": "jpg2_blocks420", "(anonymous namespace)::jpg2_hist_kernel": "jpg2_hist",
    "(anonymous namespace)::jpg2_tables_kernel": "jpg2_tables", "(anonymous namespace)::jpg2_rows_kernel": "jpg2_rows",
    "jpg2_blocks420_kernel": "jpg2_blocks420", "jpg2_hist_kernel": "jpg2_hist", "jpg2_tables_kernel": "jpg2_tables",
    "jpg2_rows_kernel": "jpg2_rows",
}


def kernel_key(name):
    """demangled rocprofv3 Kernel_Name -> the key the table is matched against"""
    return name.split("(")[0].replace("void se::", "").replace("se::", "")


def label_of(name):
    k = kernel_key(name)
    return next((v for pre, v in KERNEL_LABELS.items() if k.startswith(pre)), None)
