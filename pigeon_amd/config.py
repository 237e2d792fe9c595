"""Constants of the hot path, same names and values as reference config.py:1-92, and `TrainArgs` / `TRAIN_ARGS`: the fields of
the reference's `TRAIN_ARGS` (config.py:94-109) that the head-training loop of pigeon_amd/train.py reads.  The other
`TrainingArguments` blocks (config.py:111-177) configure training of the vision tower and are out of scope."""
from dataclasses import dataclass

# OpenAI's pretrained implementation (reference config.py:6-7)
CLIP_MODEL = 'openai/clip-vit-large-patch14-336'
CLIP_EMBED_DIM = 1024

# Geocells path (config.py:35-36)
GEOCELL_PATH = 'data/geocells_2203.csv'       # PIGEON
GEOCELL_PATH_YFCC = 'data/geocells_yfcc.csv'  # PIGEOTTO

# Country polygons of `Country_accuracy` (config.py:26)
COUNTRY_PATH = 'data/geocells/countries.geojson'

# Scaler of the six multi-task regression targets (config.py:39-40)
SCALER_PATH = 'saved_models/scaler/regression.scaler'
SCALER_PATH_YFCC = 'saved_models/scaler/regression_yfcc.scaler'

# Models (config.py:58-68)
CURRENT_SAVE_PATH = 'saved_models/WorldCLIP_head_landmarks.model'
PRETRAINED_CLIP = 'saved_models/StreetviewCLIP.model'
CLIP_PRETRAINED_HEAD = 'saved_models/New_Base_smooth_avg_MT_Geo_SV.model'
PRETRAINED_CLIP_YFCC = 'saved_models/WorldCLIP.model'
CLIP_PRETRAINED_HEAD_YFCC = 'saved_models/WorldCLIP_head.model'
CLIP_PRETRAINED_HEAD_YFCC_LANDMARKS = 'saved_models/WorldCLIP_head_landmarks.model'

# Embedding (config.py:71)
EMBED_BATCH_SIZE_PER_GPU = 512

# Evaluation batch per device (config.py:97-98: per_device_eval_batch_size=256)
EVAL_BATCH_SIZE_PER_GPU = 256

# Cluster refinement model (config.py:76-88)
PROTO_PATH = 'data/data_prototypes_2203.csv'
DATASET_PATH = 'data/hf_SVCLIP_2203'
PROTO_MODEL_PATH = 'saved_models/refiner/proto.refiner'
PROTO_PATH_YFCC = 'data/data_prototypes_YFCC.csv'
DATASET_PATH_YFCC = 'data/hf_YFCC'
PROTO_MODEL_YFCC_PATH = 'saved_models/refiner/proto_YFCC.refiner'
PROTO_PATH_LANDMARKS = 'data/data_prototypes_landmarks.csv'
DATASET_PATH_LANDMARKS = 'data/hf_landmarks'
PROTO_MODEL_LANDMARKS_PATH = 'saved_models/refiner/proto_landmarks.refiner'

# CLIP image normalisation (transformers OPENAI_CLIP_MEAN / OPENAI_CLIP_STD, used by CLIPProcessor at
# reference models/clip_embedder.py:52 and dataset_creation/finetune/embed_dataset.py:20)
OPENAI_CLIP_MEAN = [0.48145466, 0.4578275, 0.40821073]
OPENAI_CLIP_STD = [0.26862954, 0.26130258, 0.27577711]

# Geoguessr score decay (reference config.py:52) and haversine label smoothing (config.py:55)
DECAY_CONSTANT = 1492.7
LABEL_SMOOTHING_CONSTANT = 65  # (PIGEOTTO), 75 (PIGEON)


@dataclass
class TrainArgs:
    """What `pigeon_amd.train.train_model` reads from its `train_args` (any object with these fields will do; transformers'
    TrainingArguments is one).  The defaults are the values of the reference's TRAIN_ARGS (config.py:94-109)."""
    output_dir: str = 'saved_models'
    per_device_train_batch_size: int = 256
    per_device_eval_batch_size: int = 256
    num_train_epochs: int = 1000
    learning_rate: float = 2e-5
    logging_steps: int = 1
    gradient_accumulation_steps: int = 1
    seed: int = 330


TRAIN_ARGS = TrainArgs()
