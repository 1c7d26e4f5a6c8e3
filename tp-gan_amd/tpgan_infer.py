"""Inference and validation with a trained TP-GAN generator: raw photos + 68 landmarks ->
uint8 frontal faces, and PSNR / SSIM against the ground-truth frontal view.

    fz = Frontalizer.from_checkpoint("ckpt", epoch=3)        # or Frontalizer(G)
    u8 = fz(imgs, lm68)                                      # uint8 [B, 128, 128, 3]
    r = fz.evaluate(imgs, lm68, frontal)                     # fake_u8, sse, psnr, ssim
    ids = IdentityScorer(FeatureExtractModel("resnet"))      # a trained identity network
    r = fz.evaluate(imgs, lm68, frontal, identity=ids)       # ... and id_cos
    ids.enroll(gallery_u8, labels)                           # frontal views, one label each
    hit = ids.identify(fz(imgs, lm68), k=5)                  # idx, score, label [B, 5]
    cmc = ids.cmc(true_labels, hit)                          # rank-1 .. rank-5 rates
    det = LandmarkDetector.from_checkpoint("pretrain_ckpt")  # a trained MobileNetV2 + SSD head
    fz = Frontalizer(G, detector=det)
    u8 = fz(imgs)                                            # no landmarks supplied
    d = det.detect(imgs)                                     # points, score, boxes, status, ...
    al = FaceAligner(FaceAligner.template_from_landmarks(train_lm68, train_scale))
    fz = Frontalizer(G, detector=det, aligner=al)            # small, off-centre or tilted faces
    d = det.detect(imgs, aligner=al)                         # ... of the aligned faces, + matrix

The data path is FaceBatcher.from_raw (Pillow-exact LANCZOS, landmark crops, [-1, 1]), the
model is the product's Generator frozen in eval mode, the way back to pixels is
tpgan_ops.denorm_u8 and the metrics are tpgan_ops.image_metrics: everything between the
uploaded photos and the returned tensors stays on the device.  The frozen weights' bf16 / fp16
images are packed once (tpgan_ops._FrozenPack) and again only after load_state_dict.

TP-GAN is judged on identity, not pixels: IdentityScorer turns u8 faces into unit-length
embeddings of a frozen FeatureExtract.FeatureExtractModel (tpgan_ops.l2_normalize), keeps a
device-resident gallery of them and finds each probe's best matches with tpgan_ops.cosine_topk,
which never builds the probes x gallery similarity matrix.

Without landmarks, LandmarkDetector finds the four crop centres itself: LANCZOS resize,
tpgan_ops.u8_to_unit ([0, 1], what the detector was trained on), the MobileNetV2 + SSD head, and
tpgan_ops.ssd_landmarks, which decodes the head's outputs straight into FaceBatcher.from_points'
crop boxes.  One status word per face is the only thing read back.

The detector alone sees the whole photo squashed to 128 x 128, which is the generator's frame only
for a tight, upright face crop.  FaceAligner closes the gap: tpgan_ops.similarity_fit fits the
rotation + scale + translation from a template of the four points onto the detected ones, and
tpgan_ops.affine_warp_u8 resamples the photo through it (integer bilinear, sub-sampled where the
map shrinks); the detector then runs a second time on the aligned faces, whose points and boxes
are what the generator's crops use.
"""
import os
import re

import numpy as np
import torch

import D_and_G_model as DG
import tpgan_ops
from DataAndDataset import FaceBatcher


def _check_state_dict(own, sd, what):
    """Keys and shapes of sd against the model's, before anything is touched."""
    if not isinstance(sd, dict):
        raise ValueError("%s: not a state_dict (%s)" % (what, type(sd).__name__))
    if set(sd) != set(own):
        raise ValueError("%s: state_dict keys differ (missing %s, unexpected %s)" %
                         (what, sorted(set(own) - set(sd))[:5], sorted(set(sd) - set(own))[:5]))
    for k, v in sd.items():
        if tuple(v.shape) != tuple(own[k].shape):
            raise ValueError("%s: %s has shape %s, model %s" % (what, k, tuple(v.shape), tuple(own[k].shape)))


def _u8_images(device, imgs, name):
    """A [B, H, W, 3] tensor or a list of [H_i, W_i, 3] arrays / tensors -> the same on the device."""
    def one(t, what, dim):
        t = torch.as_tensor(np.ascontiguousarray(t) if isinstance(t, np.ndarray) else t)
        if t.dtype != torch.uint8 or t.dim() != dim or t.shape[-1] != 3:
            raise ValueError("%s must be uint8 %s" % (what, "[B, H, W, 3]" if dim == 4 else "[H, W, 3]"))
        return t.to(device).contiguous()
    if isinstance(imgs, (torch.Tensor, np.ndarray)) and imgs.ndim == 4:
        return one(imgs, name, 4)
    return [one(t, "%s[%d]" % (name, i), 3) for i, t in enumerate(imgs)]


def _photo_wh(imgs):
    """float64 [B, 2] (width, height) of _u8_images' result."""
    if isinstance(imgs, torch.Tensor):
        return np.array([[imgs.shape[2], imgs.shape[1]]] * imgs.shape[0], np.float64).reshape(-1, 2)
    return np.array([[t.shape[1], t.shape[0]] for t in imgs], np.float64).reshape(-1, 2)


_NAN_POINT = "cannot convert float NaN to integer: a landmark point of face(s) %s is NaN or infinite"
_BAD_ALIGN = "cannot align face(s) %s: %s"


class Frontalizer:
    """A frozen Generator behind a photo-in, pixels-out interface.

    G               a D_and_G_model.Generator.  It is moved to `device`, put in eval mode and its
                    parameters stop requiring gradients -- unless it is bound to a trainer's
                    FlatParams: such a model is used as it is (eval mode only for the duration of
                    a call), and its packed weight images keep following the optimizer.
    compute_dtype   torch.bfloat16 (default), torch.float16 or torch.float32.
    max_batch       faces per forward pass of __call__ / frontalize_batch.
    detector        a LandmarkDetector on the same device, or None.  With one, __call__ and evaluate
                    take lm68=None: the detector's four points are the crop centres.
    aligner         a FaceAligner on the same device (128 x 128 output), or None; needs a detector.
                    With one, photos without landmarks are first warped into the template's frame
                    (LandmarkDetector.detect(imgs, aligner=...)); calls that give lm68 are unchanged.
    """

    def __init__(self, G, device="cuda", compute_dtype=torch.bfloat16, max_batch=32, detector=None, aligner=None):
        if compute_dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("compute_dtype must be float32, bfloat16 or float16, got %s" % compute_dtype)
        if int(max_batch) < 1:
            raise ValueError("max_batch must be >= 1, got %s" % max_batch)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.compute_dtype = compute_dtype
        self.max_batch = int(max_batch)
        if detector is not None:
            if not isinstance(detector, LandmarkDetector):
                raise ValueError("detector must be a LandmarkDetector or None, got %s" % type(detector).__name__)
            if detector.device != self.device:
                raise ValueError("detector is on %s, the Frontalizer on %s" % (detector.device, self.device))
        self.detector = detector
        if aligner is not None:
            if not isinstance(aligner, FaceAligner):
                raise ValueError("aligner must be a FaceAligner or None, got %s" % type(aligner).__name__)
            if detector is None:
                raise ValueError("an aligner needs a detector: its points are what the faces are aligned by")
            if aligner.device != self.device:
                raise ValueError("aligner is on %s, the Frontalizer on %s" % (aligner.device, self.device))
            if aligner.out_hw != (128, 128):
                raise ValueError("the generator's frame is 128 x 128, the aligner's %s" % (aligner.out_hw,))
        self.aligner = aligner
        self.G = G
        self.zdim = G.global_pathway.zdim
        self.img_size = G.img_size
        self._trainer_bound = any(self._is_trainer_flat(getattr(p, "_tpg_flat", None)) for p in G.parameters())
        if not self._trainer_bound:
            G.to(self.device)
            G.eval()
            for p in G.parameters():
                p.requires_grad_(False)
            self._new_packs()
        self._fb = None

    @staticmethod
    def _is_trainer_flat(flat):
        return flat is not None and not isinstance(flat, tpgan_ops._FrozenPack)

    def _new_packs(self):
        # a fresh holder per parameter: images are packed on first use and kept (epoch stays 0)
        for p in self.G.parameters():
            p._tpg_flat = tpgan_ops._FrozenPack()

    @classmethod
    def from_checkpoint(cls, path, epoch=None, zdim=64, num_classes=347, use_batchnorm=False, img_size=128, **kw):
        """path: a .pth written by UtilityMethods.save_model (a bare state_dict), or a trainer
        checkpoint directory holding G/model_epoch_<epoch>.pth (epoch=None: the largest integer
        epoch there).  Loaded with weights_only=True; keys and shapes are checked before the model
        is touched."""
        if os.path.isdir(path):
            gdir = os.path.join(path, "G")
            if epoch is None:
                found = [int(m.group(1)) for m in (re.fullmatch(r"model_epoch_(\d+)\.pth", f)
                                                   for f in (os.listdir(gdir) if os.path.isdir(gdir) else [])) if m]
                if not found:
                    raise ValueError("no G/model_epoch_<epoch>.pth under %s" % path)
                epoch = max(found)
            path = os.path.join(gdir, "model_epoch_%s.pth" % epoch)
        sd = torch.load(path, map_location="cpu", weights_only=True)
        G = DG.Generator(zdim, num_classes, use_batchnorm=use_batchnorm, img_size=img_size)
        _check_state_dict(G.state_dict(), sd, "checkpoint %s" % path)
        G.load_state_dict(sd)
        return cls(G, **kw)

    def load_state_dict(self, sd):
        """New weights (checked before anything changes); the packed images follow."""
        _check_state_dict(self.G.state_dict(), sd, "load_state_dict")
        self.G.load_state_dict(sd)  # in place: the parameters keep their storage
        if self._trainer_bound:
            for flat in {id(f): f for f in (getattr(p, "_tpg_flat", None) for p in self.G.parameters())
                         if self._is_trainer_flat(f)}.values():
                with torch.cuda.device(self.device):
                    flat.weights_loaded()
        else:
            self._new_packs()

    # ---- inputs
    def _z(self, z, B):
        if z is None:
            return torch.zeros(B, self.zdim, dtype=torch.float32, device=self.device)
        if isinstance(z, torch.Generator):
            return torch.randn(B, self.zdim, generator=z, dtype=torch.float32, device=z.device).to(self.device)
        if not isinstance(z, torch.Tensor) or tuple(z.shape) != (B, self.zdim):
            raise ValueError("z must be None, a torch.Generator or a [%d, %d] tensor" % (B, self.zdim))
        return z.to(self.device, torch.float32)

    def _u8_images(self, imgs, name):
        return _u8_images(self.device, imgs, name)

    def _batcher(self):
        if self._fb is None:
            # landmark status is checked here for the whole batch, with the indices (check=False)
            self._fb = FaceBatcher(self.device, dtype=torch.float32, check=False)
        return self._fb

    # ---- forward
    def _forward_u8(self, batch, z):
        G = self.G
        was_training = G.training
        G.eval()
        try:
            with torch.no_grad(), torch.cuda.device(self.device), tpgan_ops.compute_dtype(self.compute_dtype):
                outs = G(batch["I128"], batch["left_eye"], batch["right_eye"], batch["nose"], batch["mouth"], z, False)
                return tpgan_ops.denorm_u8(outs[0])
        finally:
            if was_training:
                G.train()

    def frontalize_batch(self, batch, z=None):
        """A FaceBatcher dict ("I128" and the four patches, [-1, 1], any img_size) -> uint8 [B, S, S, 3]."""
        names = ("I128", "left_eye", "right_eye", "nose", "mouth")
        B = batch["I128"].shape[0]
        z = self._z(z, B)
        if B <= self.max_batch:
            return self._forward_u8(batch, z)
        parts = [self._forward_u8({k: batch[k][s:s + self.max_batch] for k in names}, z[s:s + self.max_batch])
                 for s in range(0, B, self.max_batch)]
        return torch.cat(parts)

    def __call__(self, imgs, lm68=None, z=None):
        """imgs: uint8 photos, a list of [H_i, W_i, 3] (any mix of sizes) or one [B, H, W, 3];
        lm68: float32 [B, 68, 2] landmarks in each photo's own pixels, or None with a detector
        attached (its four points are the crop centres) -> uint8 [B, 128, 128, 3]."""
        if self.img_size != 128:
            raise ValueError("raw photos go through FaceBatcher.from_raw, which is 128-only; this generator "
                             "has img_size %d (use frontalize_batch)" % self.img_size)
        if lm68 is None and self.detector is None:
            raise ValueError("lm68 is None and no detector is attached (Frontalizer(G, detector=...))")
        imgs = self._u8_images(imgs, "imgs")
        B = len(imgs)
        if lm68 is None:
            z = self._z(z, B)
            out = torch.empty(B, 128, 128, 3, dtype=torch.uint8, device=self.device)
            if B == 0:
                return out
            # every face's landmarks first: nothing is returned for a batch with a bad one
            d = self.detector.detect(imgs) if self.aligner is None else self.detector.detect(imgs, aligner=self.aligner)
            fb = self._batcher()
            for s in range(0, B, self.max_batch):
                e = min(B, s + self.max_batch)
                out[s:e] = self._forward_u8(fb.from_points(d["u8_128"][s:e], d["boxes"][s:e]), z[s:e])
            return out
        lm68 = torch.as_tensor(lm68)
        if lm68.dtype != torch.float32 or lm68.dim() != 3 or lm68.shape[0] != B or lm68.shape[2] != 2:
            raise ValueError("lm68 must be float32 [%d, npts, 2]" % B)
        lm68 = lm68.to(self.device).contiguous()
        z = self._z(z, B)
        out = torch.empty(B, 128, 128, 3, dtype=torch.uint8, device=self.device)
        if B == 0:
            return out
        fb = self._batcher()
        # every face's landmarks first: nothing is returned for a batch with a bad one
        wh = np.array([[t.shape[1], t.shape[0]] for t in imgs], np.float64).reshape(-1, 2)
        scale = torch.from_numpy((128.0 / wh).astype(np.float32)).to(self.device)
        status = fb.landmark_boxes(lm68, scale)[2]
        bad = torch.nonzero(status != 0).flatten().tolist()
        if bad:
            raise ValueError(_NAN_POINT % bad)
        for s in range(0, B, self.max_batch):
            e = min(B, s + self.max_batch)
            out[s:e] = self._forward_u8(fb.from_raw(imgs[s:e], lm68[s:e]), z[s:e])
        return out

    def evaluate(self, imgs, lm68, frontal, z=None, identity=None):
        """Frontalise and score against the ground-truth frontal view (uint8 [B, 128, 128, 3] on the
        device, or a list of raw photos, resized like the inputs; with an aligner and lm68=None they
        are aligned like the inputs, by the detector's points on them) -> {"fake_u8", "sse" int64 [B],
        "psnr" float64 [B] (inf where sse is 0), "ssim" float32 [B]}.  lm68 as __call__.  With identity=an
        IdentityScorer the dict also holds "id_cos" float32 [B]: the cosine similarity of the
        identity embeddings of the frontalised face and of the true frontal view."""
        if identity is not None and not isinstance(identity, IdentityScorer):
            raise ValueError("identity must be an IdentityScorer or None, got %s" % type(identity).__name__)
        fake = self(imgs, lm68, z)
        if isinstance(frontal, torch.Tensor) and frontal.dim() == 4 and tuple(frontal.shape[1:]) == (128, 128, 3):
            if frontal.dtype != torch.uint8:
                raise ValueError("frontal must be uint8 [B, 128, 128, 3] or a list of raw photos")
            real = frontal.to(self.device).contiguous()
        elif self.aligner is not None and lm68 is None:
            real = self.detector.detect(self._u8_images(frontal, "frontal"), aligner=self.aligner)["u8_128"]
        else:
            real = self._batcher().resize(self._u8_images(frontal, "frontal"), (128, 128))
        if real.shape != fake.shape:
            raise ValueError("frontal holds %d faces, imgs %d" % (real.shape[0], fake.shape[0]))
        sse, ssim = tpgan_ops.image_metrics(fake, real)
        out = {"fake_u8": fake, "sse": sse, "psnr": psnr_from_sse(sse, fake.shape[1:]), "ssim": ssim}
        if identity is not None:
            out["id_cos"] = tpgan_ops.cosine_pairs(identity.embed(fake), identity.embed(real))
        return out


def psnr_from_sse(sse, hwc):
    """10 * log10(255^2 * H * W * C / sse) in float64 on sse's device (inf where sse is 0)."""
    n = float(255 * 255) * float(hwc[0]) * float(hwc[1]) * float(hwc[2])
    return 10.0 * torch.log10(n / sse.to(torch.float64))


class IdentityScorer:
    """Identity embeddings, a gallery of them and rank-k identification, all on the device.

    extractor       a FeatureExtract.FeatureExtractModel ('resnet', 'resnet50' or 'mobilenetv2').
                    It is moved to `device`, frozen and put in eval mode; the 16-bit images of
                    its weights are packed once (tpgan_ops._FrozenPack), BatchNorm folded once.
    compute_dtype   torch.bfloat16 (default), torch.float16 or torch.float32: the extractor's
                    arithmetic.  Embeddings, similarities and the search are float32 throughout.
    max_batch       faces per extractor pass.

    An embedding is the extractor's last identity feature (pooled over the map where the
    back-end returns a map: MobileNetV2), divided by its norm.
    """

    def __init__(self, extractor, device="cuda", compute_dtype=torch.bfloat16, max_batch=32):
        if compute_dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("compute_dtype must be float32, bfloat16 or float16, got %s" % compute_dtype)
        if int(max_batch) < 1:
            raise ValueError("max_batch must be >= 1, got %s" % max_batch)
        if not hasattr(extractor, "extract_features"):
            raise ValueError("extractor must be a FeatureExtractModel (extract_features), got %s"
                             % type(extractor).__name__)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.compute_dtype = compute_dtype
        self.max_batch = int(max_batch)
        self.extractor = extractor.to(self.device).eval()
        for p in self.extractor.parameters():
            p.requires_grad_(False)
            p._tpg_flat = tpgan_ops._FrozenPack()
        self._fb = None
        self.clear()

    # ---- embeddings
    def _features(self, faces_u8):
        if self._fb is None:
            self._fb = FaceBatcher(self.device, dtype=torch.float32, check=False)
        with torch.no_grad(), torch.cuda.device(self.device), tpgan_ops.compute_dtype(self.compute_dtype):
            f = self.extractor.extract_features(self._fb.normalize(faces_u8))[-1]
            if f.dim() == 4 and (f.shape[2] != 1 or f.shape[3] != 1):
                f = tpgan_ops.global_avgpool(f)
            return f.reshape(f.shape[0], -1)

    def embed(self, faces_u8):
        """uint8 [B, S, S, 3] faces on the device -> unit-length float32 [B, D] embeddings.  A face
        whose feature holds NaN or infinity, or is all zero, raises ValueError naming it."""
        if not isinstance(faces_u8, torch.Tensor) or faces_u8.dtype != torch.uint8 or faces_u8.dim() != 4 \
                or faces_u8.shape[-1] != 3:
            raise ValueError("faces_u8 must be a uint8 [B, S, S, 3] tensor")
        if faces_u8.device != self.device:
            raise ValueError("faces_u8 must be on %s, got %s" % (self.device, faces_u8.device))
        faces_u8 = faces_u8.contiguous()
        B = faces_u8.shape[0]
        if B == 0:
            raise ValueError("faces_u8 holds no faces")
        if B <= self.max_batch:
            feats = self._features(faces_u8)
        else:
            feats = torch.cat([self._features(faces_u8[s:s + self.max_batch]) for s in range(0, B, self.max_batch)])
        unit, _, status = tpgan_ops.l2_normalize(feats, check=False)
        bad = torch.nonzero(status != 0).flatten().tolist()
        if bad:
            raise ValueError("embed: the identity feature of face(s) %s holds NaN or infinity, or is zero" % bad)
        return unit

    def _embeddings(self, x, what):
        if isinstance(x, torch.Tensor) and x.dtype == torch.uint8:
            return self.embed(x)
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.device != self.device:
            raise ValueError("%s must be uint8 [B, S, S, 3] faces or float32 [B, D] embeddings on %s"
                             % (what, self.device))
        return x

    # ---- gallery
    def clear(self):
        """Empty the gallery."""
        self._gal = None     # float32 [capacity, dpad], pad columns zero
        self._labels = None  # int64 [capacity]
        self._dim = 0
        self.size = 0

    @property
    def gallery(self):
        """The enrolled embeddings, float32 [size, D] (a view of the gallery buffer)."""
        if self._gal is None:
            raise ValueError("the gallery is empty")
        return tpgan_ops._zero_padded(self._gal[:self.size], self._dim)

    @property
    def labels(self):
        if self._gal is None:
            raise ValueError("the gallery is empty")
        return self._labels[:self.size]

    def enroll(self, faces_u8, labels):
        """Append faces (or ready embeddings) and their integer labels to the gallery; returns the
        gallery indices they were given, int64 [B]."""
        emb = self._embeddings(faces_u8, "faces_u8")
        B, D = emb.shape
        labels = torch.as_tensor(labels)
        if labels.dim() != 1 or labels.shape[0] != B or labels.is_floating_point() or labels.dtype == torch.bool:
            raise ValueError("labels must be %d integers" % B)
        labels = labels.to(self.device, torch.int64)
        if self._gal is not None and D != self._dim:
            raise ValueError("embeddings have %d columns, the gallery %d" % (D, self._dim))
        dpad = (D + 3) // 4 * 4
        need = self.size + B
        if self._gal is None or need > self._gal.shape[0]:
            cap = max(need, 2 * (self._gal.shape[0] if self._gal is not None else 0), 256)
            gal = torch.zeros(cap, dpad, dtype=torch.float32, device=self.device)
            lab = torch.full((cap,), -1, dtype=torch.int64, device=self.device)
            if self._gal is not None:
                gal[:self.size] = self._gal[:self.size]
                lab[:self.size] = self._labels[:self.size]
            self._gal, self._labels, self._dim = gal, lab, D
        self._gal[self.size:need, :D] = emb
        self._labels[self.size:need] = labels
        first, self.size = self.size, need
        return torch.arange(first, need, dtype=torch.int64, device=self.device)

    # ---- identification
    def identify(self, faces_u8, k=1, skip=None):
        """The k best gallery matches of every probe (uint8 faces or float32 [B, D] embeddings) ->
        {"idx" int32 [B, k], "score" float32 [B, k], "label" int64 [B, k]}: cosine similarity
        descending, equal scores by the lower gallery index; idx and label are -1 and score -inf
        past the number of eligible gallery rows.  skip: int32 [B], the gallery index each probe
        must not match (the probe's own enrolment), -1 for none."""
        if self._gal is None:
            raise ValueError("the gallery is empty: enroll() first")
        emb = self._embeddings(faces_u8, "faces_u8")
        if emb.shape[1] != self._dim:
            raise ValueError("embeddings have %d columns, the gallery %d" % (emb.shape[1], self._dim))
        if skip is not None:
            skip = torch.as_tensor(skip).to(self.device, torch.int32)
        idx, score = tpgan_ops.cosine_topk(emb, self.gallery, k=k, skip=skip)
        label = torch.where(idx >= 0, self.labels[idx.clamp(min=0).long()], torch.full_like(idx, -1, dtype=torch.int64))
        return {"idx": idx, "score": score, "label": label}

    @staticmethod
    def cmc(probe_labels, result):
        """Cumulative match characteristic, float64 [k] on the result's device: entry r is the
        share of probes whose own label is among their r + 1 best matches (entry 0 is rank-1)."""
        label = result["label"]
        probe_labels = torch.as_tensor(probe_labels).to(label.device, torch.int64)
        if probe_labels.dim() != 1 or probe_labels.shape[0] != label.shape[0]:
            raise ValueError("probe_labels must hold %d labels" % label.shape[0])
        if label.shape[0] == 0:
            raise ValueError("no probes")
        hit = (label == probe_labels[:, None]) & (result["idx"] >= 0)
        return (hit.cumsum(1) > 0).to(torch.float64).mean(0)


LANDMARK_NAMES = ("left_eye", "right_eye", "nose", "mouth")


class LandmarkDetector:
    """The landmark detector of the pretraining (MobileNetV2 + SSD head, Pretrain.py) as the
    generator's front end: raw photos -> the left eye, right eye, nose and mouth centre, the four
    crop centres of process(), and their crop boxes, with nothing leaving the device but one status
    word per face.

    model                 a MobileNetV2.MobileNetV2.  It is moved to `device`, frozen and put in eval
                          mode; BatchNorm is folded once and the 16-bit weight images are packed once
                          (tpgan_ops._FrozenPack), again only after load_state_dict.
    compute_dtype         torch.bfloat16 (default), torch.float16 or torch.float32: the detector's
                          arithmetic.  The decode is float32 throughout.
    max_batch             faces per detector pass.
    confidence_threshold  a landmark is found when its best softmax score is > this (MultiTaskDecoder's
                          rule and default).
    detect_hw             (height, width) the detector sees; the photos are resized to 128 x 128 first
                          (the frame the generator's crops live in), then to this size when it differs.
    on_missing            "raise": a face with a landmark that was not found fails the whole batch;
                          "best": the best-scoring anchor is used all the same and "status" says so.
    """

    def __init__(self, model, device="cuda", compute_dtype=torch.bfloat16, max_batch=32, confidence_threshold=0.5,
                 detect_hw=(128, 128), on_missing="raise"):
        if compute_dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("compute_dtype must be float32, bfloat16 or float16, got %s" % compute_dtype)
        if int(max_batch) < 1:
            raise ValueError("max_batch must be >= 1, got %s" % max_batch)
        if on_missing not in ("raise", "best"):
            raise ValueError("on_missing must be 'raise' or 'best', got %r" % (on_missing,))
        if not hasattr(model, "ssd_head") or not hasattr(model, "extra_layers"):
            raise ValueError("model must be a MobileNetV2.MobileNetV2, got %s" % type(model).__name__)
        detect_hw = (int(detect_hw[0]), int(detect_hw[1]))
        if not (32 <= detect_hw[0] <= 4096 and 32 <= detect_hw[1] <= 4096):
            raise ValueError("detect_hw sides must be in 32..4096, got %s" % (detect_hw,))
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.compute_dtype = compute_dtype
        self.max_batch = int(max_batch)
        self.confidence_threshold = float(confidence_threshold)
        self.detect_hw = detect_hw
        self.on_missing = on_missing
        self.model = model.to(self.device).eval()
        for p in self.model.parameters():
            p.requires_grad_(False)
        self._new_packs()
        self._fb = None

    def _new_packs(self):
        # a fresh holder per parameter: the folded weights and their images are made on first use
        for p in self.model.parameters():
            p._tpg_flat = tpgan_ops._FrozenPack()

    @classmethod
    def from_checkpoint(cls, path, epoch=None, **kw):
        """path: a .pth written by UtilityMethods.save_model (a bare state_dict), or the directory
        the pretraining writes model_epoch_<epoch>.pth into (epoch=None: the largest integer epoch
        there).  Loaded with weights_only=True; keys and shapes are checked before a model is touched."""
        import MobileNetV2 as MN
        if os.path.isdir(path):
            if epoch is None:
                found = [int(m.group(1)) for m in (re.fullmatch(r"model_epoch_(\d+)\.pth", f)
                                                   for f in os.listdir(path)) if m]
                if not found:
                    raise ValueError("no model_epoch_<epoch>.pth under %s" % path)
                epoch = max(found)
            path = os.path.join(path, "model_epoch_%s.pth" % epoch)
        sd = torch.load(path, map_location="cpu", weights_only=True)
        model = MN.MobileNetV2()
        _check_state_dict(model.state_dict(), sd, "checkpoint %s" % path)
        model.load_state_dict(sd)
        return cls(model, **kw)

    def load_state_dict(self, sd):
        """New weights (checked before anything changes); BatchNorm is folded and the images packed anew."""
        _check_state_dict(self.model.state_dict(), sd, "load_state_dict")
        self.model.load_state_dict(sd)  # in place: the parameters keep their storage
        self._new_packs()

    def _batcher(self):
        if self._fb is None:
            self._fb = FaceBatcher(self.device, dtype=torch.float32, check=False)
        return self._fb

    def _head(self, u8):
        """uint8 [b, h, w, 3] at detect_hw -> the head's (locations, classifications) in float32."""
        with tpgan_ops.compute_dtype(self.compute_dtype):
            loc, cls = self.model(tpgan_ops.u8_to_unit(u8, self.compute_dtype))
        return loc.float(), cls.float()

    def _decode(self, u8_128):
        """One detector pass over uint8 [B, 128, 128, 3] faces: tpgan_ops.ssd_landmarks's tuple."""
        B = u8_128.shape[0]
        dh, dw = self.detect_hw
        u8_det = u8_128 if (dh, dw) == (128, 128) else self._batcher().resize(u8_128, (dh, dw))
        heads = [self._head(u8_det[s:s + self.max_batch]) for s in range(0, B, self.max_batch)]
        loc = heads[0][0] if len(heads) == 1 else torch.cat([h[0] for h in heads])
        cls = heads[0][1] if len(heads) == 1 else torch.cat([h[1] for h in heads])
        if loc.shape[1] > 4096:
            raise ValueError("detect_hw %s gives %d anchors; the decode takes at most 4096" %
                             (self.detect_hw, loc.shape[1]))
        scale = None
        if (dh, dw) != (128, 128):
            one = (128.0 / np.array([dw, dh], np.float64)).astype(np.float32)
            scale = torch.from_numpy(np.tile(one, (B, 1))).to(self.device)
        return tpgan_ops.ssd_landmarks(loc, cls, self.confidence_threshold, scale)

    def _check_status(self, st):
        bad = [i for i, v in enumerate(st) if v & 16]
        if bad:
            raise ValueError(_NAN_POINT % bad)
        if self.on_missing == "raise":
            missing = {i: [LANDMARK_NAMES[l] for l in range(4) if v >> l & 1] for i, v in enumerate(st) if v & 15}
            if missing:
                raise ValueError("no anchor above confidence %g for face(s) %s: %s" %
                                 (self.confidence_threshold, sorted(missing),
                                  ", ".join("%d: %s" % (i, "/".join(missing[i])) for i in sorted(missing))))

    def detect(self, imgs, aligner=None):
        """imgs: uint8 photos, a list of [H_i, W_i, 3] (any mix of sizes) or one [B, H, W, 3] ->
        {"points" float32 [B, 4, 2] (x, y) of the left eye, right eye, nose and mouth centre in the
        128 x 128 frame, "points_photo" the same in each photo's own pixels (times float32 (W / 128,
        H / 128)), "score" float32 [B, 4], "anchor" int32 [B, 4], "boxes" int32 [B, 4, 4] (left, upper,
        right, lower: FaceBatcher.from_points takes them), "status" int32 [B] (tpgan_ops.ssd_landmarks),
        "u8_128" uint8 [B, 128, 128, 3]}.  The status read is the call's only copy to the host.

        aligner: a FaceAligner (128 x 128 output) or None.  With one the call is two passes: detect on
        the squashed photo as above, fit the similarity transform from the aligner's template to those
        points in the photo's own pixels and warp the photo through it, then detect again on the
        aligned faces.  The dict then describes the ALIGNED faces ("u8_128", "points", "score",
        "anchor", "boxes" and "status" are the second pass's) and adds "matrix" float32 [B, 2, 3]
        (aligned frame -> photo pixels), "align_status" int32 [B] (FaceAligner.align) and "points_photo",
        the second pass's points mapped through matrix.  on_missing and the NaN rule hold for both
        passes; a face whose fit failed (align_status bit 0 or 1) raises ValueError.  The three status
        arrays reach the host in one copy."""
        imgs = _u8_images(self.device, imgs, "imgs")
        B = len(imgs)
        if B == 0:
            raise ValueError("imgs holds no photos")
        if aligner is not None:
            if not isinstance(aligner, FaceAligner):
                raise ValueError("aligner must be a FaceAligner or None, got %s" % type(aligner).__name__)
            if aligner.device != self.device:
                raise ValueError("aligner is on %s, the detector on %s" % (aligner.device, self.device))
            if aligner.out_hw != (128, 128):
                raise ValueError("the detector's frame is 128 x 128, the aligner's %s" % (aligner.out_hw,))
        fb = self._batcher()
        with torch.no_grad(), torch.cuda.device(self.device):
            u8_128 = fb.resize(imgs, (128, 128))
            points, score, anchor, boxes, status = self._decode(u8_128)
            to_photo = torch.from_numpy((_photo_wh(imgs) / 128.0).astype(np.float32)).to(self.device)
            points_photo = points * to_photo[:, None, :]
            if aligner is None:
                st = status.tolist()  # the one device-to-host copy
            else:
                al = aligner.align(imgs, points_photo, in_status=status)
                u8_128, matrix = al["u8"], al["matrix"]
                points, score, anchor, boxes, status2 = self._decode(u8_128)
                m = matrix[:, None]  # [B, 1, 2, 3]: photo = M @ (x, y, 1)
                points_photo = points[..., 0:1] * m[..., 0] + points[..., 1:2] * m[..., 1] + m[..., 2]
                host = torch.cat([status, status2, al["status"]]).tolist()  # the one device-to-host copy
                st, st2, ast = host[:B], host[B:2 * B], host[2 * B:]
                status = status2
        self._check_status(st)
        if aligner is None:
            return {"points": points, "points_photo": points_photo, "score": score, "anchor": anchor, "boxes": boxes,
                    "status": status, "u8_128": u8_128}
        FaceAligner.check_status(ast)
        self._check_status(st2)
        return {"points": points, "points_photo": points_photo, "score": score, "anchor": anchor, "boxes": boxes,
                "status": status, "u8_128": u8_128, "matrix": matrix, "align_status": al["status"]}

    def accuracy(self, points, truth, status=None):
        """Pretrain.py's banded accuracy per face, float32 [B] (tpgan_ops.landmark_accuracy)."""
        return tpgan_ops.landmark_accuracy(points, truth, status)


class FaceAligner:
    """The step between the landmark detector and the generator: fit the similarity transform
    (rotation, uniform scale, translation) from a template of the four crop centres onto the
    points detected in a photo, and resample the photo through it, so that a small, off-centre or
    tilted face reaches the generator in the frame it was trained on.  Two launches, nothing read
    back (tpgan_ops.similarity_fit, tpgan_ops.affine_warp_u8).

    template   float32 [4, 2]: (x, y) of the left eye, right eye, nose and mouth centre in the output
               frame.  Required: derive it from the faces the generator was trained on
               (template_from_landmarks).  It must be finite and its points must not all coincide.
    out_hw     (height, width) of the aligned faces; the detector and the generator take (128, 128).
    """

    def __init__(self, template, device="cuda", out_hw=(128, 128)):
        t = template.detach().cpu().numpy() if isinstance(template, torch.Tensor) else np.asarray(template)
        if t.shape != (4, 2):
            raise ValueError("template must be float32 [4, 2], got shape %s" % (t.shape,))
        t = np.ascontiguousarray(t, np.float32)
        if not np.isfinite(t).all():
            raise ValueError("template holds a NaN or infinite coordinate")
        qc = t - t.mean(0, dtype=np.float32)
        spread = np.float32((qc * qc).sum(dtype=np.float32))
        if not (np.isfinite(spread) and spread > 0):
            raise ValueError("the template's points coincide: no scale or rotation can be fitted to them")
        out_hw = (int(out_hw[0]), int(out_hw[1]))
        if not (1 <= out_hw[0] <= 4096 and 1 <= out_hw[1] <= 4096):
            raise ValueError("out_hw sides must be in 1..4096, got %s" % (out_hw,))
        self.template = t
        self.out_hw = out_hw
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    @staticmethod
    def template_from_landmarks(lm68, scale=None):
        """The mean of the four crop centres over a set of faces -> float32 [4, 2] (numpy), in the frame
        the landmarks are in.  lm68: float32 [N, 68, 2] landmarks of training faces; scale: float32
        [N, 2] (sx, sy) per face, e.g. 128 / size for photos that are resized to 128 x 128, or None.
        The centres are FaceBatcher.landmark_boxes's reduction: float32 means of the
        FIVE_PTS_IDX_REPAIRED index ranges summed in index order, times scale, the two mouth corners
        averaged.  The mean over the faces is taken in float64 and rounded once."""
        from DataAndDataset import FIVE_PTS_IDX_REPAIRED
        lm = lm68.detach().cpu().numpy() if isinstance(lm68, torch.Tensor) else np.asarray(lm68)
        if lm.ndim != 3 or lm.shape[0] < 1 or lm.shape[1] < 55 or lm.shape[2] != 2:
            raise ValueError("lm68 must be float32 [N, 68, 2] with N >= 1, got shape %s" % (lm.shape,))
        lm = lm.astype(np.float32)
        n = lm.shape[0]
        five = np.empty((n, 5, 2), np.float32)
        for j, (lo, hi) in enumerate(FIVE_PTS_IDX_REPAIRED):
            acc = np.zeros((n, 2), np.float32)
            for i in range(lo, hi + 1):
                acc = acc + lm[:, i]
            five[:, j] = acc / np.float32(hi + 1 - lo)
        if scale is not None:
            sc = scale.detach().cpu().numpy() if isinstance(scale, torch.Tensor) else np.asarray(scale)
            if sc.shape != (n, 2):
                raise ValueError("scale must be float32 [%d, 2], got shape %s" % (n, sc.shape))
            five = five * sc.astype(np.float32)[:, None, :]
        centres = five[:, :4].copy()
        centres[:, 3] = (five[:, 3] + five[:, 4]) / np.float32(2.0)
        if not np.isfinite(centres).all():
            bad = sorted(set(np.nonzero(~np.isfinite(centres))[0].tolist()))
            raise ValueError("a landmark of face(s) %s is NaN or infinite" % bad)
        return centres.astype(np.float64).mean(0).astype(np.float32)

    @staticmethod
    def check_status(status):
        """ValueError naming the faces whose fit failed (bit 0: a point is NaN, infinite or beyond
        1e9; bit 1: the fitted transform is degenerate or out of range).  status: host ints."""
        bad = [i for i, v in enumerate(status) if v & 1]
        if bad:
            raise ValueError(_BAD_ALIGN % (bad, "a detected point is NaN, infinite or beyond 1e9"))
        bad = [i for i, v in enumerate(status) if v & 2]
        if bad:
            raise ValueError(_BAD_ALIGN % (bad, "the fitted transform is degenerate or out of range (scale zero or "
                                                "above 32, translation beyond 16384 pixels)"))

    def align(self, imgs, points_photo, in_status=None):
        """imgs: uint8 photos, a list of [H_i, W_i, 3] or one [B, H, W, 3]; points_photo: float32
        [B, 4, 2] device tensor, the four points in each photo's own pixels; in_status: int32 [B]
        (the detector's status) or None -> {"u8" uint8 [B, out_h, out_w, 3], "matrix" float32
        [B, 2, 3] (aligned frame -> photo pixels), "matrix_q16" int32 [B, 2, 3] (what the warp used),
        "status" int32 [B]: the fit's bits 0..2 ORed with the warp's bit 3 (tpgan_ops.similarity_fit,
        tpgan_ops.affine_warp_u8)}.  Nothing is read back: a face with bit 0 or 1 was warped by the
        identity, and the caller decides (check_status)."""
        imgs = _u8_images(self.device, imgs, "imgs")
        B = len(imgs)
        if not isinstance(points_photo, torch.Tensor) or points_photo.dtype != torch.float32 \
                or tuple(points_photo.shape) != (B, 4, 2):
            raise ValueError("points_photo must be a float32 [%d, 4, 2] device tensor" % B)
        if points_photo.device != self.device:
            raise ValueError("points_photo must be on %s, got %s" % (self.device, points_photo.device))
        if B == 0:
            raise ValueError("imgs holds no photos")
        with torch.no_grad(), torch.cuda.device(self.device):
            matrix, q16, fit_status = tpgan_ops.similarity_fit(points_photo, self.template, in_status)
            u8, warp_status = tpgan_ops.affine_warp_u8(imgs, q16, self.out_hw)
            return {"u8": u8, "matrix": matrix, "matrix_q16": q16, "status": fit_status | warp_status}
