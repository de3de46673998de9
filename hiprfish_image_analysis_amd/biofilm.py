"""Biofilm per-cell reports: cell_report (hiprfish_imaging_biofilm_analysis.py measure_biofilm_images_2d
:1214-1295, after the segmentation): per-cell spectra, the classifier chain with
predict_proba, regionprops shape columns, debris typing and the raw / cell-filtered barcode
adjacency matrices -- written with the reference's file names and layouts:

  {sample}_avgint.csv                  per-cell mean spectra, header 0..C-1 (:1219)
  {sample}_cell_information.csv        channel_*, intensity_classification_*, cell_barcode,
                                       max_probability, {class}_prob, sample, label, centroid_x,
                                       centroid_y, major_axis, minor_axis, eccentricity,
                                       orientation, area, epithelial_distance, max_intensity,
                                       type (:1231-1246)
  {sample}_cell_information_filtered.csv   the rows typed 'cell' (:1271-1273)
  {sample}_avgint_filtered.csv         their spectra (:1274-1275)
  {sample}_adjacency_matrix.csv / _filtered.csv   taxon code x taxon code counts (:1276-1295)

Every per-pixel and per-cell computation runs on the device (label_sums, cell_table,
backend.ClassifierModel, region_props, biofilm_typing_and_adjacency); pandas only writes.
The identification images (:1247-1258, :1260-1270: colour renderings) are not written.
The reference's script does not run as shipped (SyntaxError at :1254-1255), so
the layouts follow its source text.

measure_biofilm_2d is the whole 2-D mode (:1208-1295) from the acquisitions: registration and
segmentation (generate_2d_segmentation, :322-419) on the device, the four arrays of :1210-1213, then
cell_report.

volume_report is the same report for a segmented z-stack (measure_biofilm_images_3d, :1359-1417):
centroid_x/y/z and area for the shape columns, the sparse 3-D label adjacency, the barcode-valued
identification volumes and the Blender voxel files {sample}_identification[_filtered]_{r,g,b}.bvox
(save_identification_bvox, :280-289).
"""
from __future__ import annotations

import numpy as np
import torch

from . import kernels as K
from . import pipeline as P


def cell_report(sample: str, registered: torch.Tensor, segmentation: torch.Tensor, adjacency_seg: torch.Tensor,
                model, taxon_codes, epithelial_area: torch.Tensor | None = None, calibration=None,
                write: bool = True, area_max: float = 10000.0, prob_min: float = 0.95):
    """-> dict of DataFrames (cell_info, cell_info_filtered, avgint, avgint_filtered, adjacency,
    adjacency_filtered); `model` a backend.ClassifierModel whose barcode SVC carries probA/probB;
    `calibration` folds the flat field into the spectra as the registered image's division does"""
    import pandas as pd
    seg = segmentation.to(torch.int32).contiguous()
    maxlab = int(seg.max().item()) if seg.numel() else 0
    sums, counts = K.label_sums(registered, seg, maxlab, cal=calibration)                # :1215-1218
    _, labels, avgint, avgint_norm = K.cell_table(sums, counts, maxlab)
    feats = model.features(avgint_norm)                                                   # :1220-1226
    emb = model.umap.transform(feats).double()                                            # :1227
    cls = model.svc.predict(emb)                                                          # :1228
    prob = model.svc.predict_proba(emb)                                                   # :1229
    classes = np.asarray(model.svc.classes).astype(str)
    codes = classes[cls.cpu().numpy()]
    maxp = prob.max(dim=1).values
    props = K.region_props(seg, maxlab)[labels.long()]                                    # :1234-1241
    code_index = {c: i for i, c in enumerate(np.asarray(taxon_codes).astype(str))}
    bc_idx = torch.tensor([code_index.get(c, -1) for c in codes], dtype=torch.int32, device=seg.device)
    typ = P.biofilm_typing_and_adjacency(seg, adjacency_seg, bc_idx, len(code_index), maxp, epithelial_area,
                                         area_max, prob_min)                              # :1263-1269

    f = feats.cpu().numpy()
    C = f.shape[1] - 4
    cell_info = pd.DataFrame(f[:, :C], columns=["channel_{}".format(i) for i in range(C)])
    for i in range(4):
        cell_info["intensity_classification_{}".format(i)] = f[:, C + i]
    cell_info["cell_barcode"] = codes
    cell_info["max_probability"] = maxp.cpu().numpy()
    pr = prob.cpu().numpy()
    for k, c in enumerate(classes):
        cell_info["{}_prob".format(c)] = pr[:, k]
    cell_info["sample"] = sample
    pp = props.cpu().numpy()
    cell_info["label"] = labels.cpu().numpy()
    cell_info["centroid_x"] = pp[:, 1]
    cell_info["centroid_y"] = pp[:, 2]
    cell_info["major_axis"] = pp[:, 3]
    cell_info["minor_axis"] = pp[:, 4]
    cell_info["eccentricity"] = pp[:, 5]
    cell_info["orientation"] = pp[:, 6]
    cell_info["area"] = pp[:, 0].astype(np.int64)
    cell_info["epithelial_distance"] = 0                                                  # :1243
    cell_info["max_intensity"] = f[:, :C].max(axis=1)                                     # :1244
    is_cell = typ.is_cell.cpu().numpy().astype(bool)
    cell_info["type"] = np.where(is_cell, "cell", "debris")                               # :1245, :1268
    av = avgint.cpu().numpy()
    codes_all = np.asarray(taxon_codes).astype(str)
    out = {
        "cell_info": cell_info,
        "cell_info_filtered": cell_info.loc[is_cell, :].copy(),
        "avgint": pd.DataFrame(av),
        "avgint_filtered": pd.DataFrame(av[is_cell, :]),
        "adjacency": pd.DataFrame(typ.adjacency.cpu().numpy().astype(np.float64), index=codes_all,
                                  columns=codes_all),
        "adjacency_filtered": pd.DataFrame(typ.adjacency_filtered.cpu().numpy().astype(np.float64),
                                           index=codes_all, columns=codes_all),
    }
    if write:
        out["avgint"].to_csv("{}_avgint.csv".format(sample), index=None)                   # :1219
        out["cell_info"].to_csv(sample + "_cell_information.csv", index=None)            # :1246
        out["cell_info_filtered"].to_csv(sample + "_cell_information_filtered.csv", index=None)
        out["avgint_filtered"].to_csv("{}_avgint_filtered.csv".format(sample), index=None)
        out["adjacency"].to_csv(sample + "_adjacency_matrix.csv")                         # :1294
        out["adjacency_filtered"].to_csv(sample + "_adjacency_matrix_filtered.csv")       # :1295
    return out


def measure_biofilm_2d(sample: str, lasers, model, taxon_codes, write: bool = True, **seg_kwargs):
    """measure_biofilm_images_2d (:1208-1295) from the acquisitions of one field of view: register
    (pipeline.register_biofilm_2d, :323-346), segment (pipeline.segment_biofilm_2d, :347-418), save
    the reference's four arrays (:1210-1213)

      {sample}_registered.npy        (H, W, C) registered stack, f64 as np.zeros(image.shape) makes it
      {sample}_seg.npy               segmentation
      {sample}_adjacency_seg.npy     adjacency segmentation
      {sample}_epithelial_area.npy   bool

    and report per cell with cell_report and the epithelial area.  seg_kwargs go to
    segment_biofilm_2d (disk_radius, bkg_min_size, keep); epithelial=False is refused, the report
    needs the area.  `lasers`: the (H, W, C_l) f32 device stacks in acquisition order.
    -> cell_report's dict plus registered, segmentation, adjacency_seg, epithelial_area,
    image_registered_sum and image_final_bkg_filtered (device tensors).

    There is no command-line main: the reference's (:1419-1449) builds its taxon lookup from NCBI
    over the network (:1429); the caller passes `taxon_codes` instead."""
    if not seg_kwargs.get("epithelial", True):
        raise ValueError("measure_biofilm_2d: the report needs the epithelial area")
    registered = P.register_biofilm_2d(lasers)
    seg, n, adj, n_adj, reg_sum, final_bkg, epi = P.segment_biofilm_2d(registered, **seg_kwargs)
    if write:
        np.save("{}_registered.npy".format(sample), registered.cpu().numpy().astype(np.float64))   # :1210
        np.save("{}_seg.npy".format(sample), seg.cpu().numpy())                          # :1211
        np.save("{}_adjacency_seg.npy".format(sample), adj.cpu().numpy())                # :1212
        np.save("{}_epithelial_area.npy".format(sample), epi.cpu().numpy().astype(bool))  # :1213
    out = cell_report(sample, registered, seg, adj, model, taxon_codes, epithelial_area=epi, write=write)
    out.update(registered=registered, segmentation=seg, adjacency_seg=adj, epithelial_area=epi,
               image_registered_sum=reg_sum, image_final_bkg_filtered=final_bkg)
    return out


def write_bvox(path: str, plane: torch.Tensor):
    """one Blender voxel file (:280-289): the header [nx, ny, nz, 1] as <i4, then a (Z, Y, X) f32
    plane of paint_planes3 -- x fastest, the volume's flatten('F')"""
    nz, ny, nx = (int(d) for d in plane.shape)
    with open(path, "wb") as f:
        np.array([nx, ny, nz, 1]).astype("<i4").tofile(f)
        plane.cpu().numpy().astype("<f4", copy=False).tofile(f)


def taxon_colours(ntaxa: int) -> np.ndarray:
    """(ntaxa, 3) f32: taxon i's colorsys.hsv_to_rgb(i / ntaxa, 1, 1)"""
    import colorsys
    return np.array([colorsys.hsv_to_rgb(i / ntaxa, 1.0, 1.0) for i in range(ntaxa)], np.float32).reshape(ntaxa, 3)


def volume_report(sample: str, registered: torch.Tensor, segmentation: torch.Tensor, adjacency_seg: torch.Tensor,
                  model, taxon_codes, write: bool = True, area_max: float = 100000.0, prob_min: float = 0.95,
                  bvox: bool = True):
    """The per-cell report of a segmented z-stack (measure_biofilm_images_3d, :1359-1417): cell_report
    on an (X, Y, Z, C) registered volume, its (X, Y, Z) segmentation and adjacency segmentation.
    -> dict of DataFrames (cell_info, cell_info_filtered, avgint, avgint_filtered, adjacency,
    adjacency_filtered) and of device volumes (identification_barcode: every cell painted int(its
    barcode, 2) as :1396 does; identification_barcode_filtered: debris cells painted 0).

    Follows the reference's text: spectra per label and channel (:1363-1368), the classifier chain
    with predict_proba (:1369-1378), the columns channel_*, intensity_classification_*, cell_barcode,
    max_probability, {class}_prob, sample, label, centroid_x, centroid_y, centroid_z, area, type
    (:1379-1387), _cell_information.csv without index or header (:1389), the debris rule area >
    100000 or max_probability <= 0.95 (:1411; debris_labels is never consulted there), the colours --
    a taxon's hue, (1, 1, 1) for a barcode outside the lookup, (0.5, 0.5, 0.5) for debris in the
    filtered set (:1397-1400, :1413; taxon i's hue is i / ntaxa here, the lookup's H, S, V columns
    there) -- and the bvox layout of :280-289.  The adjacency matrices (the 2-D report's :1276-1295,
    which the 3-D function lacks) and the filtered tables are laid out as cell_report lays them out;
    the graph is rag_boundary's on the volume (connectivity 2), a sparse edge set on the device.

    The reference function does not run as shipped (segmentation, image_registered and
    image_epithelial_area are undefined in it).  Three departures from its text:
      * centroid_z is centroid[2]; :1385 repeats centroid[1];
      * the check SVCs see the StandardScaler-scaled segments, as every other report here and the
        2-D function (:1222-1226) do; the 3-D function takes no scaler argument;
      * the filtered bvox files are {sample}_identification_filtered_{r,g,b}.bvox; :1416 calls
        save_identification_bvox with the same sample and overwrites the unfiltered files.
    The identification volumes are built on the device as three f32 planes in Blender's order
    (paint_planes3); the (X, Y, Z, 3) f64 array of :1391 never exists."""
    import pandas as pd
    seg = segmentation.to(torch.int32).contiguous()
    if seg.dim() != 3 or registered.dim() != 4 or tuple(registered.shape[:3]) != tuple(seg.shape):
        raise ValueError("volume_report: an (X, Y, Z, C) volume and its (X, Y, Z) segmentation expected")
    X, Y, Z = seg.shape
    C_in = registered.shape[3]
    maxlab = int(seg.max().item()) if seg.numel() else 0
    sums, counts = K.label_sums(registered.reshape(X * Y, Z, C_in), seg.reshape(X * Y, Z), maxlab)   # :1363-1367
    _, labels, avgint, avgint_norm = K.cell_table(sums, counts, maxlab)                 # :1368
    feats = model.features(avgint_norm)                                                   # :1369-1373
    emb = model.umap.transform(feats).double()                                            # :1374
    cls = model.svc.predict(emb)                                                          # :1375
    prob = model.svc.predict_proba(emb)                                                   # :1376
    classes = np.asarray(model.svc.classes).astype(str)
    codes = classes[cls.cpu().numpy()]
    maxp = prob.max(dim=1).values                                                         # :1377
    props = K.region_props3(seg, maxlab)[labels.long()]                                   # :1381-1386
    codes_all = np.asarray(taxon_codes).astype(str)
    code_index = {c: i for i, c in enumerate(codes_all)}
    taxon = np.array([code_index.get(c, -1) for c in codes], np.int64)
    bc_idx = torch.from_numpy(taxon.astype(np.int32)).to(seg.device)
    typ = P.biofilm_typing_and_adjacency3(seg, adjacency_seg, bc_idx, len(code_index), maxp, area_max, prob_min)

    f = feats.cpu().numpy()
    C = f.shape[1] - 4
    cell_info = pd.DataFrame(f[:, :C], columns=["channel_{}".format(i) for i in range(C)])
    for i in range(4):
        cell_info["intensity_classification_{}".format(i)] = f[:, C + i]
    cell_info["cell_barcode"] = codes
    cell_info["max_probability"] = maxp.cpu().numpy()
    pr = prob.cpu().numpy()
    for k, c in enumerate(classes):
        cell_info["{}_prob".format(c)] = pr[:, k]
    cell_info["sample"] = sample
    pp = props.cpu().numpy()
    lab_host = labels.cpu().numpy()
    cell_info["label"] = lab_host
    cell_info["centroid_x"] = pp[:, 1]
    cell_info["centroid_y"] = pp[:, 2]
    cell_info["centroid_z"] = pp[:, 3]
    cell_info["area"] = pp[:, 0].astype(np.int64)
    is_cell = typ.is_cell.cpu().numpy().astype(bool)
    cell_info["type"] = np.where(is_cell, "cell", "debris")                               # :1387, :1412
    # :1392-1396: the barcode-valued volume, flat in n
    value = np.array([int(c, 2) for c in codes], np.int64).astype(np.int32)
    code_of_label = np.zeros(maxlab, np.int32)
    code_of_label[lab_host - 1] = value
    code_of_label_f = np.zeros(maxlab, np.int32)
    code_of_label_f[lab_host[is_cell] - 1] = value[is_cell]
    ident = K.paint_ids(seg, torch.from_numpy(code_of_label).to(seg.device))
    ident_f = K.paint_ids(seg, torch.from_numpy(code_of_label_f).to(seg.device))
    av = avgint.cpu().numpy()
    out = {
        "cell_info": cell_info,
        "cell_info_filtered": cell_info.loc[is_cell, :].copy(),
        "avgint": pd.DataFrame(av),
        "avgint_filtered": pd.DataFrame(av[is_cell, :]),
        "adjacency": pd.DataFrame(typ.adjacency.cpu().numpy().astype(np.float64), index=codes_all,
                                  columns=codes_all),
        "adjacency_filtered": pd.DataFrame(typ.adjacency_filtered.cpu().numpy().astype(np.float64),
                                           index=codes_all, columns=codes_all),
        "identification_barcode": ident,
        "identification_barcode_filtered": ident_f,
    }
    if write:
        out["avgint"].to_csv("{}_avgint.csv".format(sample), index=None)
        out["cell_info"].to_csv(sample + "_cell_information.csv", index=None, header=None)       # :1389
        out["cell_info_filtered"].to_csv(sample + "_cell_information_filtered.csv", index=None)
        out["avgint_filtered"].to_csv("{}_avgint_filtered.csv".format(sample), index=None)
        out["adjacency"].to_csv(sample + "_adjacency_matrix.csv")
        out["adjacency_filtered"].to_csv(sample + "_adjacency_matrix_filtered.csv")
        if bvox:
            # the colour table, (ncell + 1, 3) by label, row 0 the background (:1391 zeros)
            hue = taxon_colours(max(len(codes_all), 1))
            colour = np.zeros((maxlab + 1, 3), np.float32)
            colour[lab_host] = np.where((taxon >= 0)[:, None], hue[np.maximum(taxon, 0)], np.float32(1.0))
            colour_f = colour.copy()
            colour_f[lab_host[~is_cell]] = 0.5                                            # :1413
            for table, stem in ((colour, "_identification_"), (colour_f, "_identification_filtered_")):
                planes = K.paint_planes3(seg, torch.from_numpy(table).to(seg.device))
                for ch, name in enumerate("rgb"):
                    write_bvox("{}{}{}.bvox".format(sample, stem, name), planes[ch])
    return out
