"""Summary pictures: what a training or validation run shows of itself, made on the device.

* `color_conversion`: HSV -> RGB.
* `flow_image`: the flow wheel of a 2-D flow field and its logging call.
* `pcl_image`: pillar coordinates, the occupancy image of points, the top-down intensity image of a cloud over a variable extent.
* `bbox_image`: boxes drawn with anti-aliased lines onto bird's-eye canvases, the layered summary picture of a batch and the
  box-movement picture.
* `colormaps`: the `summer` and `gist_rainbow` tables, built here; matplotlib is not needed.

Every function takes device tensors and returns device tensors without a host read (include/liso_visu.h,
liso_amd/csrc/visu.hip), or takes numpy arrays and runs a numpy statement of the same arithmetic; each module says where the two
agree bit for bit.  A `writer` is any object with `add_images(tag, array, global_step=, dataformats=)`.

Out of scope: text on canvases (per-box text, text at a position), image grids, GIFs, PDFs, matplotlib figures, the viewer of the
box-augmentation database, and the range-view pictures (points and boxes projected onto a range image).
"""
