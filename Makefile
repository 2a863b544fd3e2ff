# Entry points of this repo.  The variable NAMES are the reference's (its `make train ...` / `make inference ...` command lines keep
# working: MODEL, DEPTHMUL, CKPT, IMG, BATCH, ...); everything else is this build's.
#
#   make build       hipcc --offload-arch=gfx950 -> k210_yolo_framework_amd/csrc/libyolo_hip.so (+ the CPU oracle used by the tests)
#   make test        CPU suite;  `python -m pytest tests -m gpu` needs an MI355X
#   make bench       images/sec, yolo_mobilev1-0.75, 32 frames per step (GPUS=N runs one rank per GPU through torchrun)
#   make inference   MODEL=... DEPTHMUL=... CKPT=weights.h5|.npz IMG=picture.jpg
#   make train       MODEL=... DEPTHMUL=... BATCH=16 MAXEP=10 [SYNTHETIC=256]
#                    [PRUNE=True INITSPARSITY=0.5 FINALSPARSITY=0.9 END_EPOCH=5 FREQUENCY=100]: magnitude pruning, saves yolo_prune_model.h5
#                    [QAT=True QATMOMENTUM=0.99 QATOBSERVE=8]: quantisation-aware fine-tuning, saves yolo_qat_model.h5 + yolo_qat_ranges.npz
#                    [BOXLOSS=giou|diou|ciou BOXWEIGHT=1.0]: an IoU-family box loss in place of the xy / wh terms (default mse: the reference's loss)
#                    [FOCAL=obj|cls|all FOCALGAMMA=2.0 FOCALALPHA=0.25 LABELSMOOTH=0.1 OBJTARGET=iou]: focal loss on the objectness and / or class
#                    terms, smoothed class targets, the IoU of the predicted box as an object cell's objectness target (all off by default: the
#                    reference's loss; the values named here are starting points, not findings: DESIGN.md 3.25, profiles/lossopt_*.txt)
#                    [MOSAIC=True MOSAICPROB=1.0 MOSAICOFF=0]: four pictures per training sample, composed on the GPU; the last MOSAICOFF epochs without
#                    [HSV=True HSVHUE=0.1 HSVSAT=1.5 HSVEXP=1.5 HSVPROB=1.0]: HSV colour jitter of every training frame, on the GPU (Darknet's recipe)
#                    [TEACHERCKPT=big.h5|.npz TEACHER=yolo_mobilev2 TEACHERDEPTH=1.0 DISTILLWEIGHT=1.0]: knowledge distillation from a trained network of
#                    the zoo with the same IMGSIZE, OUTSIZE, anchors and CLSNUM (TEACHER / TEACHERDEPTH default to MODEL / DEPTHMUL): per raw output the
#                    Bernoulli KL from the teacher's sigmoid to the student's, classes and box scaled by the teacher's objectness, squared error on
#                    the wh logits; the step and epoch lines then name the `distill` term.  Empty TEACHERCKPT (default): off.  The wh term is
#                    unbounded where the teacher's wh logits are wild, and DISTILLWEIGHT=1.0 is a starting point: DESIGN.md 3.18, profiles/distill_*.txt
#                    [CACHE=gpu CACHEGB=8 CACHESTAGE=256]: every training picture is decoded once and kept in device memory (CACHEGB GB; what does
#                    not fit is brought in every epoch through staging regions of CACHESTAGE MB, which must hold the uncached pictures of one
#                    batch); every batch is composed from there by one launch and the epoch line names the hits / misses: DESIGN.md 3.19
#                    [DECODE=gpu]: the pictures that still have to be decoded are, if baseline JPEG files, decoded on the GPU into that
#                    memory by the project's own integer rule (not PIL's bytes: DESIGN.md 3.12), every other file by PIL; works without CACHE=gpu
#                    [EMA=True EMADECAY=0.9999 EMATAU=2000]: an exponential moving average of the weights (decay ramped over EMATAU updates) is
#                    validated and saved as yolo_ema_model.h5 beside the usual checkpoint; [CLIPNORM=10.0]: global-norm gradient clipping (0: off);
#                    [LRSCHED=cosine|step|constant WARMUP=N LRFINAL=0.01]: linear warmup and a schedule over the whole run: DESIGN.md 3.21
#                    [LABELS=gpu]: the label grids are built on the GPU from the boxes; [ASSIGN=multi ASSIGNIOU=0.213]: every anchor that fits a box better than ASSIGNIOU is trained on it: DESIGN.md 3.26
#   make kmodel      CKPT=yolo_model.h5 OUT=yolo.kmodel|.kfpkg [SYNTHETIC=256 | CALIB=data/voc_img_ann.npy]: 8-bit K210 model, calibrated on the GPU
#                    [RANGES=yolo_qat_ranges.npz]: the ranges a QAT run learned instead of a calibration
#                    [CALIBMETHOD=minmax|percentile|mse CALIBPCT=99.99 CALIBBINS=2048]: minmax (default) takes each tensor's exact range; percentile
#                    and mse clip it from a histogram taken on the GPU in a second pass over the calibration images (not with RANGES=)
#                    [EQUALIZE=True EQMAXGAIN=64]: cross-layer range equalisation first (k210_yolo_framework_amd/equalize.py): one more pass
#                    measures every conv output per channel on the GPU, the weights are rewritten so that the channels of a tensor fill its
#                    range, and the file is that network - the same function, other weights (not with RANGES=; default off)
#                    [BIASCORRECT=True]: per-channel bias correction after the calibration (k210_yolo_framework_amd/biascorrect.py): on the same
#                    images, one KPU-exact statistics pass per conv layer finds the integer to add to every channel's bn_add so that its mean
#                    pre-activation equals the float network's (not with RANGES=: it needs frames; default off)
#                    [ADAROUND=True ADAITERS=1000 ADALAMBDA=0.01 ADALR=0.01]: adaptive weight rounding after the calibration and before the bias
#                    correction (k210_yolo_framework_amd/adaround.py): every kernel weight takes its lower or upper code so that each output
#                    channel's error over the calibration images falls (not with RANGES=: it needs frames; default off)
#                    [ANALYZE=True ANALYZESEED=S ANALYZETOP=3]: after the file is written, the finished kmodel is measured against the float network
#                    conv by conv on the GPU (k210_yolo_framework_amd/qerror.py): accumulated and local SQNR, cosine, mean and largest error in
#                    codes, share of codes at 0 and 255, the ANALYZETOP worst channels; one table row per conv and OUT.qerror.json; on the
#                    calibration images, or with SYNTHETIC=N ANALYZESEED=S on N generated images of seed S (not with RANGES=: no frames; default off)
#   make eval        CKPT=yolo_model.h5|yolo.kmodel [PRECISION=f16x2|f16|kpu] [ANN=data/voc_img_ann.npy | SYNTHETIC=256] [EVALOBJ=0.05] [VOC07=True]:
#                    VOC mAP of the checkpoint, network and metric on the GPU; prints the per-class AP table, writes eval.json beside CKPT
#                    [METRIC=coco]: also the COCO-style AP (IoU .50:.95, AP50, AP75, small / medium / large, AR) and a `coco` object in eval.json
#                    [CURVES=True CONF=0.6 CURVESTEPS=1000 CURVESOUT=curves.npz]: also precision / recall / F1 per class at CONF and at each class's
#                    best-F1 threshold, the threshold with the best mean F1 and the confusion matrix at CONF; an `operating` object in eval.json
#                    (make train VALMAP=True appends val_mAP to every epoch line)
#                    [TTA=flip|v5|1,0.83f,0.67 TTATHRESH=0.55]: test-time augmentation, every picture also mirrored / shrunk, the views' rows fused on the GPU
#   make detect      CKPT=yolo_model.h5|yolo.kmodel SRC=folder|list.txt [OUTDIR=out] [DRAW=True|False] [PRECISION=...] [DECODE=pil|gpu] [ENCODE=pil|gpu QUALITY=75]: every
#                    picture of SRC through the pipeline; writes OUTDIR/detections.json and, with DRAW=True, OUTDIR/<stem>_res.jpg (boxes and
#                    labels drawn on the GPU; ENCODE=gpu also JPEG-encodes them there at QUALITY, ENCODE=pil leaves that to PIL on the host;
#                    DECODE=gpu decodes baseline JPEG files there too, by the project's own integer rule, every other file by PIL)
#                    [TTA=flip|v5|1,0.83f,0.67 TTATHRESH=0.55]: test-time augmentation, every picture also mirrored / shrunk, the views' rows fused on the GPU
#   make anchors     DATASET=voc ANCNUM=3 [LOW='0.0 0.0' HIGH='1.0 1.0']   (reference Makefile:78-87: k-means anchors from data/<set>_img_ann.npy)
#                    [ANCDEVICE=gpu RESTARTS=256 ANCSEED=0]: RESTARTS random starts in one GPU call; the set with the highest mean IoU is
#                    kept and that IoU printed (ANCDEVICE=cpu RESTARTS=N loops the same rule in numpy)

PY            ?= python3
MODEL         ?= yolo_mobilev1
DEPTHMUL      ?= 0.75
CLSNUM        ?= 20
DATASET       ?= voc
IMGSIZE       ?= 224 320
OUTSIZE       ?= 7 10 14 20
OBJTHRESH     ?= 0.7
IOUTHRESH     ?= 0.5
# inference, detect, eval: the decode's suppression rule, hard | linear | gaussian | diou (train VALMAP=True stays on hard)
NMS           ?= hard
NMSSIGMA      ?= 0.5
# detect, eval: sliced inference, TILES=NXxNY runs every picture as overlapping tiles (+ the whole picture with TILEFULL=True) and merges
# the rows on the GPU (k210_yolo_framework_amd/tiles.py); empty = off
TILES         ?=
TILEOVERLAP   ?= 0.2
TILEFULL      ?= True
TILEMATCH     ?= ios
TILETHRESH    ?= 0.5
# detect, eval: test-time augmentation, TTA=a comma list of gains in (0, 1], f appended for a mirrored view (flip = 1,1f; v5 = 1,0.83f,0.67):
# every picture runs once per view and the rows are fused by Weighted Boxes Fusion on the GPU (k210_yolo_framework_amd/tta.py); empty = off
TTA           ?=
TTATHRESH     ?= 0.55
CKPT          ?= ""
IMG           ?= data/synthetic_320x224.jpg
# training only
BATCH         ?= 32
MAXEP         ?= 10
ILR           ?= 0.0005
LRDECAYFACTOR ?= 0
OBJWEIGHT     ?= 1
NOOBJWEIGHT   ?= 1
WHWEIGHT      ?= 1
SPLITFACTOR   ?= 0.05
IAA           ?= False
PRUNE         ?= False
INITSPARSITY  ?= 0.5
FINALSPARSITY ?= 0.9
END_EPOCH     ?= 5
FREQUENCY     ?= 100
SYNTHETIC     ?= 0
QAT           ?= False
QATMOMENTUM   ?= 0.99
QATOBSERVE    ?= 8
VALMAP        ?= False
BOXLOSS       ?= mse
BOXWEIGHT     ?= 1.0
FOCAL         ?=
FOCALGAMMA    ?= 2.0
FOCALALPHA    ?= 0
LABELSMOOTH   ?= 0
OBJTARGET     ?=
MOSAIC        ?= False
MOSAICPROB    ?= 1.0
MOSAICOFF     ?= 0
HSV           ?= False
HSVHUE        ?= 0.1
HSVSAT        ?= 1.5
HSVEXP        ?= 1.5
HSVPROB       ?= 1.0
TEACHERCKPT   ?=
TEACHER       ?=
TEACHERDEPTH  ?=
DISTILLWEIGHT ?= 1.0
CACHE         ?= off
CACHEGB       ?= 8
CACHESTAGE    ?= 256
EMA           ?= False
EMADECAY      ?= 0.9999
EMATAU        ?= 2000
CLIPNORM      ?= 0
LRSCHED       ?=
WARMUP        ?= 0
LRFINAL       ?= 0.01
LABELS        ?= host
ASSIGN        ?= best
ASSIGNIOU     ?= 0.213
# eval only
PRECISION     ?= f16x2
ANN           ?= data/$(DATASET)_img_ann.npy
EVALOBJ       ?= 0.05
VOC07         ?= False
METRIC        ?=
CURVES        ?= False
CONF          ?= 0.6
CURVESTEPS    ?= 1000
CURVESOUT     ?=
# detect only
SRC           ?= data
OUTDIR        ?= out
DRAW          ?= True
ENCODE        ?= pil
DECODE        ?= pil
QUALITY       ?= 75
# kmodel only
OUT           ?= yolo.kmodel
CALIB         ?= data/$(DATASET)_img_ann.npy
RANGES        ?=
CALIBMETHOD   ?=
CALIBPCT      ?= 99.99
CALIBBINS     ?= 2048
EQUALIZE      ?= False
EQMAXGAIN     ?= 64
BIASCORRECT   ?= False
ADAROUND      ?= False
ADAITERS      ?= 1000
ADALAMBDA     ?= 0.01
ADALR         ?= 0.01
ANALYZE       ?= False
ANALYZESEED   ?=
ANALYZETOP    ?= 3
GPUS          ?= 1
# anchors only (reference Makefile:27-29)
ANCNUM        ?= 3
LOW           ?= 0.0 0.0
HIGH          ?= 1.0 1.0
ANCDEVICE     ?= cpu
RESTARTS      ?= 1
ANCSEED       ?=

NET_ARGS   = --train_set $(DATASET) --class_num $(CLSNUM) --model_def $(MODEL) --depth_multiplier $(DEPTHMUL) \
             --image_size $(IMGSIZE) --output_size $(OUTSIZE) --obj_thresh $(OBJTHRESH) --iou_thresh $(IOUTHRESH)
# (nothing for the default rule: the command lines of the three targets stay what they were)
NMS_ARGS   = $(if $(filter-out hard,$(NMS)),--nms $(NMS) --nms_sigma $(NMSSIGMA))
TILE_ARGS  = $(if $(TILES),--tiles $(TILES) --tile_overlap $(TILEOVERLAP) --tile_full $(TILEFULL) --tile_match $(TILEMATCH) --tile_thresh $(TILETHRESH))
TTA_ARGS   = $(if $(TTA),--tta $(TTA) --tta_thresh $(TTATHRESH))
TRAIN_ARGS = --pre_ckpt $(CKPT) --augmenter $(IAA) --batch_size $(BATCH) --rand_seed 3 --max_nrof_epochs $(MAXEP) \
             --init_learning_rate $(ILR) --learning_rate_decay_factor $(LRDECAYFACTOR) --obj_weight $(OBJWEIGHT) \
             --noobj_weight $(NOOBJWEIGHT) --wh_weight $(WHWEIGHT) --vaildation_split $(SPLITFACTOR) --log_dir log \
             --is_prune $(PRUNE) --prune_initial_sparsity $(INITSPARSITY) --prune_final_sparsity $(FINALSPARSITY) \
             --prune_end_epoch $(END_EPOCH) --prune_frequency $(FREQUENCY) --synthetic $(SYNTHETIC) \
             --qat $(QAT) --qat_momentum $(QATMOMENTUM) --qat_observe $(QATOBSERVE) --val_map $(VALMAP) \
             --box_loss $(BOXLOSS) --box_weight $(BOXWEIGHT) --mosaic $(MOSAIC) --mosaic_prob $(MOSAICPROB) --mosaic_off_epochs $(MOSAICOFF) \
             --hsv $(HSV) --hsv_hue $(HSVHUE) --hsv_sat $(HSVSAT) --hsv_exposure $(HSVEXP) --hsv_prob $(HSVPROB) \
             --cache $(CACHE) --cache_gb $(CACHEGB) --cache_stage_mb $(CACHESTAGE) --decode $(DECODE) \
             $(if $(TEACHERCKPT),--teacher_ckpt $(TEACHERCKPT) --distill_weight $(DISTILLWEIGHT) $(if $(TEACHER),--teacher_def $(TEACHER)) \
             $(if $(TEACHERDEPTH),--teacher_depth $(TEACHERDEPTH))) \
             $(if $(filter True,$(EMA)),--ema True --ema_decay $(EMADECAY) --ema_tau $(EMATAU)) \
             $(if $(filter-out 0 0.0,$(CLIPNORM)),--clip_norm $(CLIPNORM)) \
             $(if $(filter-out host,$(LABELS)),--labels $(LABELS)) $(if $(filter-out best,$(ASSIGN)),--assign $(ASSIGN) --assign_iou $(ASSIGNIOU)) \
             $(if $(LRSCHED),--lr_schedule $(LRSCHED) --warmup_steps $(WARMUP) --lr_final $(LRFINAL))$(if \
             $(filter-out off,$(FOCAL))$(filter-out 0 0.0,$(LABELSMOOTH))$(filter-out label,$(OBJTARGET)), --focal $(or $(FOCAL),off) \
             --focal_gamma $(FOCALGAMMA) --focal_alpha $(FOCALALPHA) --label_smooth $(LABELSMOOTH) --obj_target $(or $(OBJTARGET),label))
ifeq ($(GPUS),1)
LAUNCH = $(PY)
else
LAUNCH = $(PY) -m torch.distributed.run --nnodes=1 --nproc-per-node $(GPUS) --master-addr 127.0.0.1 --master-port 29533
endif

.PHONY: all build test bench inference train anchors kmodel eval detect
all:
	@echo 'targets: build | test | bench | inference | train | kmodel | eval | detect   (see the header of this Makefile)'

build:
	$(PY) -c "import __graft_entry__ as g; g.build()"

test:
	$(PY) -m pytest tests -x -q -m "not gpu"

bench:
	$(LAUNCH) bench.py --gpus $(GPUS)

inference:
	$(PY) keras_inference.py $(CKPT) $(IMG) $(NET_ARGS) $(NMS_ARGS)

train:
	$(LAUNCH) keras_train.py $(NET_ARGS) $(TRAIN_ARGS)

# the step the reference leaves to keras_freeze.py + nncase: CKPT -> 8-bit kmodel; SYNTHETIC=N calibrates on generated images
kmodel:
	$(PY) make_kmodel.py $(CKPT) $(OUT) --train_set $(DATASET) --class_num $(CLSNUM) --model_def $(MODEL) --depth_multiplier $(DEPTHMUL) \
		--image_size $(IMGSIZE) --output_size $(OUTSIZE) $(if $(RANGES),--ranges $(RANGES),$(if $(filter-out 0,$(SYNTHETIC)),--synthetic $(SYNTHETIC),--calib $(CALIB))) \
		$(if $(CALIBMETHOD),--calib_method $(CALIBMETHOD) --calib_percentile $(CALIBPCT) --calib_bins $(CALIBBINS))$(if $(filter True,$(EQUALIZE)), --equalize True --equalize_max_gain $(EQMAXGAIN))$(if $(filter True,$(BIASCORRECT)), --bias_correct True)$(if $(filter True,$(ADAROUND)), --adaround True --adaround_iters $(ADAITERS) --adaround_lambda $(ADALAMBDA) --adaround_lr $(ADALR))$(if $(filter True,$(ANALYZE)), --analyze True --analyze_top $(ANALYZETOP)$(if $(ANALYZESEED), --analyze_seed $(ANALYZESEED)))

# VOC mAP of CKPT (.h5 / .npz, or .kmodel / .kfpkg with PRECISION=kpu) on the validation head of ANN, or on SYNTHETIC=N generated images
eval:
	$(PY) keras_eval.py $(CKPT) --train_set $(DATASET) --class_num $(CLSNUM) --model_def $(MODEL) --depth_multiplier $(DEPTHMUL) \
		--image_size $(IMGSIZE) --output_size $(OUTSIZE) --iou_thresh $(IOUTHRESH) --precision $(PRECISION) --obj_thresh $(EVALOBJ) \
		--voc07 $(VOC07) $(if $(filter-out 0,$(SYNTHETIC)),--synthetic $(SYNTHETIC),--ann $(ANN)) $(if $(METRIC),--metric $(METRIC)) $(NMS_ARGS) $(TILE_ARGS) $(TTA_ARGS) \
		$(if $(filter True,$(CURVES)),--curves True --conf_thresh $(CONF) --curve_steps $(CURVESTEPS) $(if $(CURVESOUT),--curves_out $(CURVESOUT)))

# every picture of SRC (a folder or a text list) -> OUTDIR/detections.json + OUTDIR/<stem>_res.jpg; batches of BATCH pictures of any sizes
detect:
	$(PY) keras_detect.py $(CKPT) $(SRC) --out_dir $(OUTDIR) --draw $(DRAW) --decode $(DECODE) --encode $(ENCODE) --quality $(QUALITY) --batch $(BATCH) --precision $(PRECISION) $(NET_ARGS) $(NMS_ARGS) $(TILE_ARGS) $(TTA_ARGS)

# reference Makefile:78-87 (same flags; --is_random True as there)
anchors:
	$(PY) ./make_anchor_list.py $(DATASET) --max_iters 10 --is_random True --in_hw $(IMGSIZE) --out_hw $(OUTSIZE) --anchor_num $(ANCNUM) \
		--low $(LOW) --high $(HIGH) --device $(ANCDEVICE) --restarts $(RESTARTS) $(if $(ANCSEED),--seed $(ANCSEED))
