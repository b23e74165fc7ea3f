"""Enhance a file or a folder: the reference's demo.py and eval.py in one script.  Every image file of --input (or the one
file) goes through hvi_cidnet_amd.enhance_folder -- decode, upload as bytes, ingest kernel, model, egress kernel, download as
bytes, encode, pipelined -- and is saved to --output_dir under its own name.  Prints one JSON line built from the report.

    python tools/enhance.py --input datasets/LOLdataset/eval15/low --output_dir output/LOLv1 --weight weights/LOLv1/w_perc.pth
    python tools/enhance.py --input photo.jpg --output_dir out --weight weights/generalization.safetensors --gamma 0.8 --alpha_s 1.1
    python tools/enhance.py --input photos/ --output_dir out --weight weights/generalization.safetensors --tile 1024
    python tools/enhance.py --input photos/ --output_dir out --weight weights/generalization.safetensors --ensemble 8

--tile N cuts every image into overlapping N x N windows, runs them through the model --tile_batch at a time and blends the
overlaps: for images too large for one pass, or folders whose images all differ in size.  The model's channel attention is
global, so a tiled result is not the whole-image result.
--ensemble N (2, 4 or 8) is geometric self-ensemble: the model runs on N flipped / transposed views of every image and the
results, mapped back, are averaged (2: the image and its mirror; 4: all flips; 8: the flips and their transposes).  N forwards
per image; not combined with --tile.
--png device encodes the .png outputs on the device (row filters and Huffman coding, no match search) and leaves the host only
the framing: the same pixels in another valid file, smaller than Pillow's on photographs and larger on flat synthetic images.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"base": "CIDNet", "mssa": "CIDNet_MSSA", "tnsm": "CIDNet_TNSM"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input", required=True, help="an image file, or a directory of image files")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--weight", required=True, help=".pth state_dict, .safetensors, or a directory holding model.safetensors")
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="base")
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--alpha_s", type=float, default=1.3)
    ap.add_argument("--alpha_i", type=float, default=1.0)
    ap.add_argument("--gated", action="store_true")
    ap.add_argument("--gated2", action="store_true")
    ap.add_argument("--batch_size", type=int, default=1)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--tile", type=int, default=None, help="tile side, a multiple of 8 (default: the whole image in one pass)")
    ap.add_argument("--tile_overlap", type=int, default=32, help="pixels two neighbouring tiles share (at most half a tile)")
    ap.add_argument("--tile_batch", type=int, default=8, help="tiles per model launch")
    ap.add_argument("--ensemble", type=int, choices=(1, 2, 4, 8), default=1, help="views averaged per image (default 1: none)")
    ap.add_argument("--png", choices=("pillow", "device"), default="pillow", help="who encodes .png outputs (default pillow)")
    ap.add_argument("--jpeg", choices=("pillow", "device"), default="pillow",
                    help="who encodes .jpg / .jpeg outputs (default pillow; device writes the same bytes)")
    a = ap.parse_args(argv)
    if a.ensemble != 1 and a.tile is not None:
        ap.error("--ensemble and --tile cannot be combined")
    if not os.path.exists(a.input):
        ap.error(f"--input {a.input}: no such file or directory")

    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    if not torch.cuda.is_available():
        sys.exit("tools/enhance.py needs a ROCm device: the package has no CPU path")
    model = getattr(P, VARIANTS[a.variant])()
    missing, unexpected = P.load_weights(model, a.weight)
    model = model.to("cuda:0").eval()
    if os.path.isdir(a.input):
        files = M.folder_images(a.input)
    else:                                                        # a single file goes through the same driver
        files = M.FolderImages([a.input], [os.path.basename(a.input)])
    if len(files) == 0:
        sys.exit(f"no image file (.png .jpg .bmp .JPG .jpeg) in {a.input}")
    rep = P.enhance_folder(model, files, a.output_dir, gamma=a.gamma, gated=a.gated, alpha_s=a.alpha_s, gated2=a.gated2,
                           alpha=a.alpha_i, batch_size=a.batch_size, threads=a.threads, depth=a.depth, tile=a.tile,
                           overlap=a.tile_overlap, tile_batch=a.tile_batch, ensemble=a.ensemble, png=a.png, jpeg=a.jpeg)
    wall = rep.seconds["wall"]
    print(json.dumps({"what": "enhance", "input": a.input, "output_dir": a.output_dir, "variant": a.variant, "images": len(rep.names),
                      "batches": len(rep.batches), "seconds": rep.seconds, "images_per_s": len(rep.names) / wall if wall > 0 else None,
                      "missing_keys": missing, "unexpected_keys": unexpected, "names": rep.names,
                      "sizes": [list(s) for s in rep.sizes], "tile": a.tile, "tiles": rep.tiles, "ensemble": rep.ensemble,
                      "png": rep.png, "jpeg": rep.jpeg, "jpeg_second_copies": rep.jpeg_second_copies}))


if __name__ == "__main__":
    main()
