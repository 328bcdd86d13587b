"""BASELINE configs[4]: "End-to-end: GLMNet + Seq2Seq (PyTorch-ROCm) -> HIP UNet3D 50-step -> VAE decode, sub1 synthetic EEG,
40-concept sweep" -- the whole generation flow of the reference (EEG2Video/inference_eeg2video.py:60-98 with the Seq2Seq / DANA
latents of EEG2Video_New) over 40 concepts x 5 clips, batched and shardable over ranks:

    raw EEG [B,62,200] ----GLMNet (host torch; --glmnet native: HIP)--> fast / slow label -> DANA's dynamic_beta (0.3 / 0.2)
    DE features [B,310] ---Semantic Predictor (HIP)--> cond [B,77,768]      (--features native: DE of the clip's raw [62,400] segment, HIP)
    EEG windows [B,7,62,100] --Seq2Seq (host torch)--> latents [B,6,4,36,64] --DANA noise + layout fix (HIP)--> [B,4,6,36,64]
    e2v_generate (HIP: 50 x [UNet3D on 2B samples, CFG, DDIM] + VAE decode) -> frames -> uint8 (HIP) -> GIF / NPY writer (host)

Synthetic EEG and random-init weights throughout (no datasets / checkpoints offline).  Prints one JSON line: clips/s of the
whole flow and the share of each stage.  ``--tiny`` runs the same code on the tiny test configuration in seconds.
``--score-against DIR`` scores every clip against ``DIR/<concept>_<k>.npy`` (or ``.gif``) as the reference's
``40_class_run_metrics.py:284-298`` does -- per-frame SSIM and MSE (``e2v_frame_metrics``), on the device while the batch's frames
are still there -- and adds ``ssim_mean``, ``ssim_std``, ``mse_mean`` and a ``score`` stage to the line.
``--classifier DIR`` (with ``--score-against``; a LOCAL ``google/vit-base-patch16-224`` checkpoint directory) adds that script's image
accuracy (``:302-328``: ``img_classify_metric`` at 2 and 40 ways, 100 trials, seeded here) as ``image_2way_acc`` / ``image_40way_acc``:
the ViT classifier of every generated and ground-truth frame runs in the score stage (``e2v_image_classify``).
``--video-classifier DIR`` (with ``--score-against``; a LOCAL ``MCG-NJU/videomae-base-finetuned-kinetics`` checkpoint directory) adds
its video accuracy (``:332-374``: ``video_classify_metric`` at 2 and 40 ways) as ``video_2way_acc`` / ``video_40way_acc``: the VideoMAE
classifier of every generated and ground-truth clip, built for the sweep's frame count, runs next to it (``e2v_video_classify``).
``--clip-model DIR`` (with ``--score-against``; a LOCAL ``openai/clip-vit-base-patch32`` checkpoint directory) adds its CLIP score
(``:20-55,145-188``): ``clip_score_mean`` over the frames (``clip_score_only``) and the frame-level N-way CLIP accuracy
``clip_2way_acc`` / ``clip_40way_acc`` (``n_way_scores``: 10 trials, top 1, seeded here; a sweep of fewer frames than ways leaves that
key out).  Both sides' frames are embedded in the score stage (``e2v_clip_embed``); one ``e2v_clip_similarity`` matrix at the end holds
every score the trials ask for.

    python examples/run_sweep.py --dtype bf16 --batch 32            # 200 clips on one GPU
    python -m torch.distributed.run --nproc-per-node 8 examples/run_sweep.py   # concepts sharded over ranks, frames gathered
"""
import argparse, json, os, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def load_clip(stem):
    """``stem + '.npy'`` or ``stem + '.gif'`` as ``save_videos_grid`` wrote it -> uint8 ``[F,H,W,3]``"""
    if os.path.isfile(stem + ".npy"):
        a = np.load(stem + ".npy")
    else:
        from PIL import Image, ImageSequence
        with Image.open(stem + ".gif") as im:
            a = np.stack([np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(im)])
    if a.ndim != 4 or a.dtype != np.uint8:
        raise ValueError(f"{stem}: expected uint8 frames [F,H,W,3], got {a.dtype} {a.shape}")
    return a


def main(argv=None, engine=None):
    """``engine``: an already built full-size ``Engine`` (tests reuse one; its semantic-predictor weights are (re)loaded here)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--concepts", type=int, default=40)
    ap.add_argument("--per-concept", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8, help="clips per e2v_generate call")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--seq2seq", default="host", choices=["host", "native"],
                    help="the Seq2Seq stage: host (default) -- the plain-torch look-alike of host_models --, or native -- the reference's "
                         "myTransformer on the device (e2v_seq2seq_latents; synthetic weights, fp32 whatever --dtype)")
    ap.add_argument("--glmnet", default="host", choices=["host", "native"],
                    help="the GLMNet stage: host (default) -- the plain-torch look-alike of host_models --, or native -- the reference's "
                         "glfnet on the device (e2v_glmnet_raw; synthetic weights, fp32 whatever --dtype)")
    ap.add_argument("--features", default="synthetic", choices=["synthetic", "native"],
                    help="the Semantic Predictor's input: synthetic (default) -- a noise draw per clip --, or native -- the DE features of the "
                         "clip's own synthetic raw 2-s segment [62, 400] (e2v_eeg_de_psd, a fixed seeded scaler), whose first 200 samples then "
                         "serve the GLMNet stage; adds a `features` stage; under --tiny the semantic predictor takes 310 inputs")
    ap.add_argument("--out", default="", help="directory for <concept>_<k>.gif (empty: frames are produced but not written)")
    ap.add_argument("--npy", action="store_true", help="write .npy instead of .gif")
    ap.add_argument("--score-against", default="", metavar="DIR",
                    help="directory of ground-truth clips named as --out names them (.npy or .gif): per-frame SSIM / MSE on the device")
    ap.add_argument("--classifier", default="", metavar="DIR",
                    help="with --score-against: local ViTForImageClassification checkpoint directory -> image_{2,40}way_acc")
    ap.add_argument("--video-classifier", default="", metavar="DIR",
                    help="with --score-against: local VideoMAEForVideoClassification checkpoint directory -> video_{2,40}way_acc")
    ap.add_argument("--clip-model", default="", metavar="DIR",
                    help="with --score-against: local CLIPVisionModelWithProjection checkpoint directory -> clip_score_mean, clip_{2,40}way_acc")
    ap.add_argument("--metric-dtype", default="fp32", choices=["fp32", "bf16", "fp16"],
                    help="arithmetic of the metric models given above (fp16: what the reference runs them in; fp32: the default)")
    args = ap.parse_args(argv)
    if args.clip_model and not args.score_against:
        ap.error("--clip-model scores against ground truth: give --score-against DIR too")
    if args.classifier and not args.score_against:
        ap.error("--classifier scores against ground truth: give --score-against DIR too")
    if args.video_classifier and not args.score_against:
        ap.error("--video-classifier scores against ground truth: give --score-against DIR too")

    import torch.distributed as dist
    from eeg2video_amd.dist import all_gather_frames, shard_range
    from eeg2video_amd.engine import Engine
    from eeg2video_amd.host_models import GLMNet, Seq2SeqLatents
    from eeg2video_amd.semantic import CLIP
    from eeg2video_amd.util import save_videos_grid
    from eeg2video_amd.weights import (TINY_UNET, TINY_VAE, GLMNetConfig, SemanticConfig, Seq2SeqConfig, UNetConfig, VAEConfig, counter_normal,
                                       counter_uniform, synth_state_dict, unet_param_spec, vae_param_spec)

    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    native_de = args.features == "native"
    ucfg, vcfg, scfg = ((TINY_UNET, TINY_VAE, SemanticConfig(in_features=310 if native_de else 22, hidden=96, tokens=77)) if args.tiny
                        else (UNetConfig(), VAEConfig(), SemanticConfig()))
    F, h, w = (3, 4, 6) if args.tiny else (6, 36, 64)
    # --seq2seq native: the reference's model over the sweep's [7, 62, 100] windows, its latent and steps those of the sweep
    s2s_cfg = None
    if args.seq2seq == "native":
        s2s_cfg = (Seq2SeqConfig(d_model=64, heads=4, ffn=128, encoder_layers=1, decoder_layers=2, steps=F, latent=(4, h, w)) if args.tiny
                   else Seq2SeqConfig(steps=F, latent=(4, h, w)))
    # --glmnet native: the reference's glfnet(2, 64, 62, 200) alone (no feature model)
    glm_cfg = GLMNetConfig(mlp_out=0) if args.glmnet == "native" else None
    t_setup = time.perf_counter()
    if engine is not None:
        eng = engine
    else:
        eng = Engine(ucfg, vcfg, local, sem_cfg=scfg, seq2seq_cfg=s2s_cfg, glmnet_cfg=glm_cfg)
        eng.load_state_dict(synth_state_dict(unet_param_spec(ucfg), seed=42, mode="reference_init"))
        eng.load_state_dict(synth_state_dict(vae_param_spec(vcfg), seed=43, mode="reference_init"), prefix="vae.")
        eng.finalize(Engine.UNET | Engine.VAE)
    sem = CLIP(scfg, engine=eng)
    if getattr(eng, "_sweep_sem_seed", None) != 44:                 # (a reused engine keeps the 0.89 G synthetic parameters)
        sem.init_synthetic(44)
        eng._sweep_sem_seed = 44
    eng.set_compute_dtype(args.dtype)
    dev = eng.device
    torch.manual_seed(0)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if glm_cfg is None:
        glm = GLMNet(out_dim=2, emb_dim=64, C=62, T=200).to(dev).eval()
    else:                                                           # on the sweep's engine where it was built for the model, else on one of its own
        from eeg2video_amd.glmnet import glfnet
        glm = glfnet(2, 64, 62, 200, config=glm_cfg, engine=eng if eng.glmnet_cfg == glm_cfg else None, device=local).init_synthetic(48)
    de_scaler = None
    if native_de:                                                   # a StandardScaler's mean_ / scale_ over the 310 features, fixed and seeded
        de_scaler = (t_(10.0 + counter_normal(45, "de_mean", (310,))).to(dev), t_(1.0 + counter_uniform(46, "de_scale", 310)).to(dev))
    if s2s_cfg is None:
        s2s = Seq2SeqLatents(d_model=512 if not args.tiny else 64, latent_shape=(4, h, w), frames=F).to(dev).eval()
    else:                                                           # on the sweep's engine where it was built for the model, else on one of its own
        from eeg2video_amd.seq2seq import myTransformer
        native = myTransformer(s2s_cfg, engine=eng if eng.seq2seq_cfg == s2s_cfg else None, device=local).init_synthetic(47)
        s2s = lambda x: native.predict_latents(x, layout="bfchw")   # [B, F, 4, h, w], as the host stage returns it
    t_setup = time.perf_counter() - t_setup

    total = args.concepts * args.per_concept
    lo, hi = shard_range(total, rank, world)                       # clips partition over ranks, no data-path exchange
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    neg = t(counter_normal(2, "neg", (1, scfg.tokens, ucfg.cross_attention_dim))).to(dev)
    stage = {"glmnet": 0.0, "seq2seq": 0.0, "semantic": 0.0, "dana": 0.0, "generate": 0.0, "uint8_d2h": 0.0, "write": 0.0}
    mine, scores, classes, video_classes, clip_embeds = [], [], [], [], []
    if native_de:
        stage["features"] = 0.0
    if args.score_against:
        stage["score"] = 0.0
    vit = None
    if args.classifier:
        from eeg2video_amd.image_classifier import ViTForImageClassification
        vit = ViTForImageClassification.from_pretrained(args.classifier, device=local,       # its own context; --dtype does not reach it
                                                        compute_dtype=args.metric_dtype)
    vmae = None
    if args.video_classifier:                                       # built for the sweep's frame count, as the reference passes num_frames
        from eeg2video_amd.video_classifier import VideoMAEForVideoClassification
        vmae = VideoMAEForVideoClassification.from_pretrained(args.video_classifier, num_frames=F, device=local, compute_dtype=args.metric_dtype)
    clipm = None
    if args.clip_model:
        from eeg2video_amd.clip_vision import CLIPVisionModelWithProjection
        clipm = CLIPVisionModelWithProjection.from_pretrained(args.clip_model, device=local, compute_dtype=args.metric_dtype)
    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0)) - 2)))
    pending = []

    def tick(name, t0):
        torch.cuda.synchronize()
        stage[name] += time.perf_counter() - t0

    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for b0 in range(lo, hi, args.batch):
        ids = list(range(b0, min(b0 + args.batch, hi)))
        B = len(ids)
        # synthetic "sub1" recordings of these clips (seeded by the clip id: any rank reproduces any clip)
        win = torch.stack([t(counter_normal(2000 + k, "win", (7, 62, 100))) for k in ids]).to(dev)
        if native_de:                                               # the clip's 2-s segment: its DE features, and its first 200 samples below
            seg = torch.stack([t(counter_normal(1000 + k, "segment", (62, 400))) for k in ids]).to(dev)
            t0 = time.perf_counter()
            de = eng.eeg_de_psd(seg, samples=400, strides=(62 * 400, 0, 400), batch=B, windows=1, electrodes=62, scaler=de_scaler,
                                psd=False)[0].reshape(B, 310)
            tick("features", t0)
            raw = seg[:, :, :200].contiguous() if glm_cfg is None else seg
        else:
            raw = torch.stack([t(counter_normal(1000 + k, "raw", (62, 200))) for k in ids]).to(dev)
            de = torch.stack([t(counter_normal(3000 + k, "de", (scfg.in_features,))) for k in ids]).to(dev)
        t0 = time.perf_counter()
        if glm_cfg is None:
            with torch.no_grad():
                fast = glm(raw[:, None]).argmax(1).bool()           # fast / slow optical-flow class -> dynamic_beta
        else:
            fast = glm.predict(raw).bool()                          # (a segment is read through its electrode stride: the first 200 samples)
        tick("glmnet", t0)
        t0 = time.perf_counter()
        lat_s2s = s2s(win).float()                                  # [B, F, 4, h, w]
        tick("seq2seq", t0)
        t0 = time.perf_counter()
        cond = sem(de).reshape(B, scfg.tokens, -1)
        tick("semantic", t0)
        t0 = time.perf_counter()
        e_div, e_same = torch.empty(lat_s2s.shape), torch.empty((B, 1) + tuple(lat_s2s.shape[2:]))
        for j, k in enumerate(ids):                                 # DANA's two draws, seeded per clip: batching never changes a clip
            g = torch.Generator().manual_seed(4000 + k)
            e_div[j] = torch.randn(lat_s2s.shape[1:], generator=g)
            e_same[j] = torch.randn((1,) + tuple(lat_s2s.shape[2:]), generator=g)
        lat = torch.empty((B, 4, F, h, w), device=dev)
        for flag, beta in ((True, 0.3), (False, 0.2)):             # DANA's two dynamic_beta values, one kernel call per group
            sel = (fast == flag).nonzero().flatten()
            if sel.numel():
                cpu = sel.cpu()
                lat[sel] = eng.dana_noise(lat_s2s[sel], e_div[cpu], e_same[cpu], t=[499] * int(sel.numel()), dynamic_beta=beta)
        tick("dana", t0)
        t0 = time.perf_counter()
        frames = eng.generate(lat, cond, neg, args.steps, 12.5, 0.0, decode=True)
        tick("generate", t0)
        if args.score_against:
            names = [f"{k // args.per_concept:02d}_{k % args.per_concept}" for k in ids]
            gt = torch.from_numpy(np.stack([load_clip(os.path.join(args.score_against, nm)) for nm in names])).to(dev)   # [B,F,H,W,3] uint8
            t0 = time.perf_counter()
            scores.append(eng.frame_metrics(frames, gt, b_channels_last=True))
            if vit is not None:                                     # probabilities of the generated frames, top 3 of the ground truth
                classes.append((vit.classify(frames, channels_last=False)[1], vit.classify(gt, channels_last=True)[2]))
            if vmae is not None:                                    # the same per clip
                video_classes.append((vmae.classify(frames, channels_last=False)[1], vmae.classify(gt, channels_last=True)[2]))
            if clipm is not None:                                   # embeddings of both sides, per frame
                clip_embeds.append((clipm.embed(frames, channels_last=False), clipm.embed(gt, channels_last=True)))
            tick("score", t0)
        t0 = time.perf_counter()
        u8 = eng.frames_to_uint8(frames).cpu()
        tick("uint8_d2h", t0)
        mine.append(u8)
        if args.out:
            # the GIF encoder (Pillow's quantiser, ~0.45 s per clip on one core) runs on a worker pool while the GPU generates
            # the next batch; "write" = the time the main thread spent waiting for it at the end
            for j, k in enumerate(ids):
                name = f"{k // args.per_concept:02d}_{k % args.per_concept}" + (".npy" if args.npy else ".gif")
                pending.append(pool.submit(save_videos_grid, u8[j:j + 1], os.path.join(args.out, name)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in pending:
        f.result()
    stage["write"] += time.perf_counter() - t0
    pool.shutdown()
    elapsed = time.perf_counter() - t_all
    u8_all = torch.cat(mine) if mine else torch.zeros((0, 3, F, 8 * h, 8 * w), dtype=torch.uint8)
    score_keys = {}
    if args.score_against:
        ssim = torch.cat([s for s, _ in scores]).cpu() if scores else torch.zeros((0, F))
        mse = torch.cat([m for _, m in scores]).cpu() if scores else torch.zeros((0, F))
        if world > 1:                                               # per-frame scores of every rank, in clip order
            parts = [None] * world
            dist.all_gather_object(parts, (ssim, mse))
            ssim, mse = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        ssim, mse = ssim.double().numpy(), mse.double().numpy()
        score_keys = {"ssim_mean": float(np.mean(ssim)), "ssim_std": float(np.std(ssim)), "mse_mean": float(np.mean(mse))}
        for what, clf, pairs in (("image", vit, classes), ("video", vmae, video_classes)):
            if clf is None:
                continue
            from eeg2video_amd.metrics import n_way_top_k_acc
            probs = torch.cat([p for p, _ in pairs]).cpu() if pairs else torch.zeros((0, clf.config.num_labels))
            top3 = torch.cat([g for _, g in pairs]).cpu() if pairs else torch.zeros((0, 3), dtype=torch.int32)
            if world > 1:
                parts = [None] * world
                dist.all_gather_object(parts, (probs, top3))
                probs, top3 = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            for n_way in (2, 40):                                   # 40_class_run_metrics.py:302-374: 100 trials, top 1, per frame / per clip
                np.random.seed(n_way)
                acc = [n_way_top_k_acc(p, [int(i) for i in g], n_way, 100, 1)[0] for p, g in zip(probs.numpy(), top3.numpy())]
                score_keys[f"{what}_{n_way}way_acc"] = float(np.mean(acc)) if acc else float("nan")
        if clipm is not None:
            from eeg2video_amd.metrics import n_way_from_matrix
            D = clipm.config.projection_dim
            pe = torch.cat([p for p, _ in clip_embeds]).cpu() if clip_embeds else torch.zeros((0, D))
            ge = torch.cat([g for _, g in clip_embeds]).cpu() if clip_embeds else torch.zeros((0, D))
            if world > 1:
                parts = [None] * world
                dist.all_gather_object(parts, (pe, ge))
                pe, ge = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            if len(pe):
                t0 = time.perf_counter()
                matrix = clipm.engine.clip_similarity(pe, ge, matrix=True).cpu().numpy()       # the pair scores are its diagonal, bit for bit
                stage["score"] += time.perf_counter() - t0
                score_keys["clip_score_mean"] = float(np.mean([float(v) for v in np.diagonal(matrix)]))
                for n_way in (2, 40):
                    if n_way <= len(pe):
                        np.random.seed(n_way)
                        score_keys[f"clip_{n_way}way_acc"] = float(np.mean(n_way_from_matrix(matrix, n_way, 1, 10)))
    if world > 1:
        u8_all = all_gather_frames(u8_all.to(dev).float() / 255.0, as_uint8=True).cpu()
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = tt.item()
    if rank == 0:
        assert u8_all.shape == (total, 3, F, 8 * h, 8 * w) and u8_all.dtype == torch.uint8
        host = stage["glmnet"] + stage["seq2seq"]
        print(json.dumps({"workload": f"{args.concepts} concepts x {args.per_concept} clips, {args.steps}-step DDIM, CFG 12.5, {F}x{8 * h}x{8 * w}, {args.dtype}, batch {args.batch}",
                          "clips": total, "n_gpus": world, "seconds": elapsed, "clips_per_s": total / elapsed, "setup_s": t_setup,
                          "stage_seconds_rank0": stage, "host_model_share": host / max(elapsed, 1e-9),
                          "generate_share": stage["generate"] / max(elapsed, 1e-9), "uint8_checksum": int(u8_all.long().sum()), **score_keys}))
    if world > 1:
        dist.destroy_process_group()
    return u8_all


if __name__ == "__main__":
    main()
