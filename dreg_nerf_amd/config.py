"""Command-line flags of the registration entry points: names and defaults follow conerf/utils/config.py:4-146
(only the flags the registration path reads are kept; unknown reference flags are accepted and ignored)."""
import argparse


def config_parser(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--local_rank", type=int, default=0)
    p.add_argument("--distributed", action="store_true")
    p.add_argument("--seed", type=int, default=3407)
    p.add_argument("--epochs", type=int, default=50)
    p.add_argument("--max_iterations", type=int, default=20000)
    p.add_argument("--num_process", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--finetune", action="store_true")
    p.add_argument("--dataset", type=str, default="")
    p.add_argument("--json_dir", type=str, default="")
    p.add_argument("--data_split_json", type=str, default="")
    p.add_argument("--factor", type=int, default=4)
    p.add_argument("--train_split", type=str, default="trainval")
    p.add_argument("--root_dir", type=str, default="")
    p.add_argument("--scene", type=str, default="")
    p.add_argument("--expname", type=str, default="chair_reg")
    p.add_argument("--aabb", type=lambda s: [float(v) for v in s.split(",")], default="-1.5,-1.5,-1.5,1.5,1.5,1.5")
    p.add_argument("--test_chunk_size", type=int, default=8192)
    p.add_argument("--unbounded", action="store_true")
    p.add_argument("--multi_blocks", action="store_true")
    p.add_argument("--position_embedding_type", type=str, default="sine")
    p.add_argument("--position_embedding_dim", type=int, default=256)
    p.add_argument("--position_embedding_scaling", type=float, default=1.0)
    p.add_argument("--num_downsample", type=int, default=6)
    p.add_argument("--robust_loss", action="store_true")
    p.add_argument("--ckpt_path", type=str, default="")
    p.add_argument("--no_load_opt", action="store_true")
    p.add_argument("--no_load_scheduler", action="store_true")
    p.add_argument("--enable_tensorboard", action="store_true")
    p.add_argument("--enable_visdom", action="store_true")
    p.add_argument("--n_tensorboard", type=int, default=30)
    p.add_argument("--n_validation", type=int, default=2500)
    p.add_argument("--n_checkpoint", type=int, default=5000)
    # build-side additions
    p.add_argument("--precision", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--pairs_per_step", type=int, default=1, help="pairs per optimizer step and GPU (reference: 1)")
    p.add_argument("--synthetic", type=int, default=0, help="use N synthetic shell-R scenes instead of a dataset on disk")
    p.add_argument("--synthetic_res", type=int, default=128)
    p.add_argument("--backward", type=str, default="rays", choices=["rays", "samples"],
                   help="train_ngp_nerf.py: the training backward: the ray kernel (dreg_ngp_render_bwd) or the sample list (dreg_ngp_render_train_samples, "
                        "dreg_ngp_samples_grad, dreg_ngp_points_bwd; DESIGN.md 3o), which also carries opacity and depth gradients")
    p.add_argument("--opacity_loss_weight", type=float, default=0.0,
                   help="train_ngp_nerf.py --backward samples: weight of mean((opacity - alpha)^2) over all rays of the batch, alpha the images' own "
                        "alpha channel (0 = off; the weight is not tuned)")
    p.add_argument("--dump_outputs", action="store_true",
                   help="eval: per scene, transformation_est.json and the registration's point clouds as PLY files (eval_nerf_regtr.py:313-438)")
    p.add_argument("--render_views", action="store_true",
                   help="eval: per scene, render both NeRF blocks under the ground-truth, predicted and no alignment (render_videos, eval_nerf_regtr.py:113-172,345-369)")
    p.add_argument("--render_merged", action="store_true",
                   help="eval: per scene, render both NeRF blocks as ONE scene (fused two-block renderer) under the ground-truth and the predicted pose, and write "
                        "PSNR / SSIM between the two to merged_metrics.json (the photometric cost of the pose error; needs the block checkpoints)")
    p.add_argument("--eval_images", action="store_true",
                   help="eval_ngp_nerf.py: render the held-out views of --scene and write PSNR / SSIM per view to eval/<scene>/[block_k/]metrics.json (evaluate, eval_ngp_nerf.py:159-244 of the reference)")
    p.add_argument("--point_cloud", action="store_true",
                   help="eval_ngp_nerf.py: depth-range point cloud of the block's training cameras, point_cloud.ply next to the checkpoint (generate_point_cloud, eval_ngp_nerf.py:246-334 of the reference)")
    p.add_argument("--fgr_baseline", action="store_true",
                   help="also run the Fast Global Registration baseline on every pair and write fgr_metrics_{split}.json (eval_nerf_regtr.py:303-311 of the reference)")
    p.add_argument("--refine_pose", action="store_true",
                   help="eval_nerf_regtr.py: refine every predicted pose by point-to-plane ICP on the two voxel point clouds (fused kernels, DESIGN.md 3f; the reference's "
                        "refine_registration, global_registration.py:85-93) and write refined_metrics_{split}.json next to metrics_{split}.json, which is unchanged")
    p.add_argument("--icp_max_dist", type=float, default=0.05, help="--refine_pose: correspondence distance threshold")
    p.add_argument("--icp_iters", type=int, default=30, help="--refine_pose: iteration limit")
    p.add_argument("--icp_normals", type=str, default="field", choices=["field", "pca"],
                   help="--refine_pose: target normals from the target block's density gradient (needs the block's checkpoint, else PCA) or by neighbourhood PCA")
    p.add_argument("--ransac_pose", action="store_true",
                   help="eval_nerf_regtr.py: also estimate every pose robustly from the predicted correspondences (fused RANSAC kernels + consensus refits, "
                        "DESIGN.md 3g) and write ransac_metrics_{split}.json next to metrics_{split}.json, which is unchanged; with --refine_pose ICP is run "
                        "from that pose as well (ransac_refined_metrics_{split}.json)")
    p.add_argument("--ransac_thresh", type=float, default=0.05, help="--ransac_pose: inlier distance (round 0's voxel-average cell and ICP's default gate; not tuned)")
    p.add_argument("--ransac_hyps", type=int, default=16384, help="--ransac_pose: number of minimal-sample hypotheses")
    p.add_argument("--ransac_seed", type=int, default=0, help="--ransac_pose: seed of the triplet draw")
    p.add_argument("--ransac_min_overlap", type=float, default=0.0, help="--ransac_pose: drop correspondences whose predicted overlap score is below this")
    p.add_argument("--normals", action="store_true",
                   help="eval_ngp_nerf.py --point_cloud: also write the field's normals (-grad density, normalised) at the points into point_cloud.ply")
    p.add_argument("--mesh", action="store_true",
                   help="eval_ngp_nerf.py: instead of the grid extraction, write mesh.ply next to every block's model.pth: the iso-surface of the block's density "
                        "at --mesh_level by the fused marching-cubes kernels (DESIGN.md 3h; the reference's convert_sdf_samples_to_ply, utils.py:284-344), with the "
                        "field's normals and mean colours; prints V, F, area and volume")
    p.add_argument("--mesh_resolution", type=int, default=256, help="--mesh / --merged_mesh: cells per axis of the lattice that spans the block's aabb")
    p.add_argument("--mesh_level", type=float, default=None,
                   help="--mesh / --merged_mesh: density of the iso-surface (default 0.7, the grid extraction's density mask; whether that gives the best-looking "
                        "surface on trained scenes has not been measured)")
    p.add_argument("--merged_mesh", action="store_true",
                   help="eval_nerf_regtr.py: per scene whose block checkpoints are on disk, write merged_mesh_pred.ply and merged_mesh_gt.ply: the source block's mesh "
                        "moved by the predicted / the known pose, concatenated with the target block's")
    p.add_argument("--merged_mesh_field", action="store_true",
                   help="eval_nerf_regtr.py: per scene whose block checkpoints are on disk, mesh the registered pair as ONE density field (fused pair-density "
                        "kernel, DESIGN.md 3i; --mesh_resolution cells on the pair's longest axis, --mesh_level) under the predicted and the known pose: "
                        "merged_field_mesh_pred.ply, merged_field_mesh_gt.ply and merged_field_mesh.json (V, F, area, volume of both)")
    p.add_argument("--register_scene", action="store_true",
                   help="eval_nerf_regtr.py: after the normal pass, register every scene as a WHOLE: all ordered pairs of its blocks through the network, pose "
                        "synchronisation into one pose per block (dreg_nerf_amd/pose_graph.py, DESIGN.md 3j), scene_metrics_{split}.json next to "
                        "metrics_{split}.json, which is unchanged")
    p.add_argument("--scene_robust", action="store_true",
                   help="--register_scene: re-solve with the edges reweighted by their residuals, w0 / (1 + (theta / 2 deg)^2 + (|t| / 0.05)^2), ten rounds; "
                        "neither scale is tuned (0.05 is round 0's voxel-average cell and ICP's default gate)")
    p.add_argument("--synthetic_blocks", type=int, default=2,
                   help="--synthetic with --register_scene / --render_scene: blocks per synthetic scene, 2 to 4 (another value ends the run before anything is evaluated)")
    p.add_argument("--render_scene", action="store_true",
                   help="eval_nerf_regtr.py: implies --register_scene (the whole registration runs and scene_metrics_{split}.json is written); then, per scene whose block checkpoints are on disk, render ALL its blocks as one scene (fused K-block "
                        "renderer, DESIGN.md 3j) from every block's cameras under the ground-truth and the synchronised poses, and write PSNR / SSIM between the "
                        "two to scene_render_metrics.json")
    p.add_argument("--scene_mesh_field", action="store_true",
                   help="eval_nerf_regtr.py: implies --register_scene; then, per scene whose block checkpoints are on disk, mesh ALL its blocks as ONE density field "
                        "(fused K-block density kernel, DESIGN.md 3k; --mesh_resolution cells on the scene's longest axis, --mesh_level) under the ground-truth "
                        "and the synchronised poses: scene_field_mesh_gt.ply, scene_field_mesh_aligned.ply and scene_field_mesh.json (K; V, F, area, volume of both)")
    p.add_argument("--scene_voxel_grid", action="store_true",
                   help="eval_nerf_regtr.py: implies --register_scene; then, per scene whose block checkpoints are on disk, extract ALL its blocks as ONE voxel grid "
                        "(fused K-block radiance kernel, DESIGN.md 3l; --scene_grid_resolution cells per axis over the scene's box) under the ground-truth and the "
                        "synchronised poses: scene_voxel_grid_{gt,aligned}.pt, scene_voxel_mask_{gt,aligned}.pt (the format of a block's voxel_grid.pt / "
                        "voxel_mask.pt), the kept samples as .ply and scene_voxel_grid.json (K, resolution, box, kept cells, IoU of the two kept sets)")
    p.add_argument("--scene_grid_resolution", type=int, default=128, help="--scene_voxel_grid: cells per axis of the merged voxel grid")
    p.add_argument("--merge_scene", action="store_true",
                   help="eval_nerf_regtr.py: implies --register_scene; then, per scene whose block checkpoints are on disk, distil ALL its blocks into ONE NeRF "
                        "block per pose set (field distillation on points, DESIGN.md 3m): merged_block_{gt,aligned}/model.pth in the format of a "
                        "train_ngp_nerf.py checkpoint, and merged_block.json (K, steps, points, final loss, PSNR / SSIM against the K-block render)")
    p.add_argument("--merge_iterations", type=int, default=2000, help="--merge_scene: distillation steps (untuned)")
    p.add_argument("--merge_points", type=int, default=65536, help="--merge_scene: points per distillation step (untuned)")
    p.add_argument("--refine_scene", action="store_true",
                   help="eval_nerf_regtr.py: implies --register_scene; then every scene's synchronised poses are refined JOINTLY by point-to-plane ICP over all "
                        "ordered block pairs at once (fused K-block kernels, DESIGN.md 3n; --icp_max_dist, --icp_iters, --icp_normals apply): "
                        "scene_refined_metrics_{split}.json, and the scene products of the same run take the refined poses")
    p.add_argument("--photo_refine", action="store_true",
                   help="eval_nerf_regtr.py: after the normal pass, refine every scene's pose photometrically (analysis by synthesis through the field's input "
                        "gradients, DESIGN.md 3p) from the ICP-refined pose when --refine_pose is also given, else from the predicted pose, per scene whose "
                        "block checkpoints are on disk: photo_refined_metrics_{split}.json next to metrics_{split}.json, which is unchanged")
    p.add_argument("--photo_iters", type=int, default=200, help="--photo_refine: Adam iterations (not tuned)")
    p.add_argument("--photo_rays", type=int, default=4096, help="--photo_refine: rays per iteration and direction (not tuned)")
    p.add_argument("--photo_lr", type=float, default=2e-3, help="--photo_refine: Adam's learning rate on the twist (not tuned)")
    p.add_argument("--photo_depth_weight", type=float, default=0.1, help="--photo_refine: weight of the depth term of the loss (not tuned)")
    p.add_argument("--eval_batch", type=int, default=4, help="eval: pairs per forward call (reference: 1; results per scene do not depend on it beyond bf16 rounding)")
    p.add_argument("--extract_grids", action="store_true",
                   help="eval_nerf_regtr.py: extract the voxel grids of the split's NeRF blocks first (what eval_ngp_nerf.py does, same files) and register from the device-resident grids, pipelined")
    p.add_argument("--pose_loss_weight", type=float, default=0.0,
                   help="train: weight of an opt-in pose loss (mean L1 of the source key points moved by the predicted vs the true pose); 0 = the reference's step")
    p.add_argument("--pose_loss_layers", type=str, default="last", choices=["last", "all"],
                   help="train: decoder layers the pose loss supervises (the reference's losses read the last one)")
    p.add_argument("--min_num_blocks", type=int, default=2, help="train_ngp_nerf.py --multi_blocks: fewest camera-cluster blocks per scene")
    p.add_argument("--max_num_blocks", type=int, default=2, help="train_ngp_nerf.py --multi_blocks: most camera-cluster blocks per scene")
    args, _unknown = p.parse_known_args(argv)
    if isinstance(args.aabb, str):
        args.aabb = [float(v) for v in args.aabb.split(",")]
    return args
