"""Feature store <-> dense feature matrix.

An existing bliss-rs SQLite library (`Library`, src/library.rs) keeps one row per (song, feature index) in the table
`feature(song_id, feature real, feature_index)` next to `song(id, path, ..., version, analyzed, ...)`
(src/library.rs:500-531).  The playlist / pairwise kernels want an n x d f32 matrix; these helpers move between the
two without re-analysing anything:

    load_feature_matrix   the read path of `songs_from_library` (src/library.rs:1355-1372): songs with
                          analyzed = true and version = ?, ordered by song id, features ordered by feature_index
    load_songs            the same rows as `Song` objects (metadata + Analysis)
    store_song            the write path of `store_song` (src/library.rs:1560-1630): upsert the song row, replace
                          its feature rows
    create_schema         the two tables, for new databases (user_version = the number of migrations)
    upgrade               `Library::upgrade` (src/library.rs:631-681): brings a database written by an older bliss-rs to
                          the current schema (track_number text -> integer, disc_number, training_triplet,
                          version not null default 1), keyed on `pragma user_version` like the crate

and the reference's library playlists (`Library::songs_from_library` / `song_from_path` / `songs_from_album` /
`playlist_from` / `playlist_from_custom` / `album_playlist_from`, src/library.rs:762-893, 1355-1460) as functions of a
database:

    songs_from_library, song_from_path, songs_from_album
    playlist_from, playlist_from_custom   seeds first, seeds removed from the pool by path, the order and ONE
                                          deduplication of the whole chain on the device (playlist.dedup_order)
    album_playlist_from                   closest_album_to_group, cropped after `number_albums` album changes
    album_playlists                       album_playlist_from for EVERY album (or artist, genre, saved playlist) of the
                                          library: one database read, one device call (playlist.nearest_albums)
    similar_songs                         the k closest songs of every song (or of some), one device call
                                          (playlist.nearest_order): playlist_from(&[song]).take(k) for the whole library
    duplicate_songs                       the groups of songs that are the same song by the rule of dedup_playlist
                                          (closer than the threshold, or the same title and artist) over EVERY pair of the
                                          library, one device call (playlist.duplicate_labels); nothing is deleted
    cluster_songs                         the k groups the library falls into (k-means on the device, playlist.cluster_songs),
                                          every group's songs with the most typical first
    training_triplets, store_training_triplet   the crate's `training_triplet` table ("song_1 and song_2 are closer together
                                          than they are to odd_one_out", src/library.rs:542-556) as row indices, and a writer
    learn_metric                          a Mahalanobis M for MahalanobisBuilder, learned on the device from those triplets
                                          or from triplets drawn from genre / album / artist / cluster labels
    similar_groups, similar_artists,      which artists (albums, genres) are like each other under the average nearest-member
    similar_artists_playlist              distance (playlist.group_neighbours), one device call for every key; and the
                                          "similar artists to the current one" playlist of the reference's TODO.md
    song_tree, linked_clusters, tour      the library's minimum spanning tree (playlist.minimum_spanning_tree, one device
                                          call): clusters without a number of clusters and of any shape, and every song
                                          (or one genre's) in an order in which each sounds like one before it
    song_map                              a picture of the library: a point per song on a plane where sonic neighbours are
                                          neighbours (playlist.song_map: exact t-SNE, every iteration on the device)
    store_fingerprints, load_fingerprints,   acoustic fingerprints (bliss_rs_amd.fingerprint_batch) in a sidecar table the crate
    fingerprint_duplicates                ignores, and the groups of songs that are the same RECORDING by them: candidates from
                                          the k nearest songs by features and equal title and artist, one match call on the
                                          device (playlist.fingerprint_duplicates); duplicate_songs is unchanged
    store_loudness, load_loudness,        EBU R 128 loudness (bliss_rs_amd.loudness_batch) in a sidecar table the crate ignores:
    loudness_statistics                   track and album loudness and peaks for ReplayGain, the loudness range, and the
                                          library's count, mean and extrema of both (host arithmetic over the table)

SQLite stores `real` as f64; an f32 feature widens exactly on the way in and narrows exactly on the way out, so a
round trip is bit-exact.  The schema, load and store helpers are host code; the playlists run their distances on the
GPU like the rest of the playlist module.
"""
import sqlite3
from typing import List, Sequence, Tuple, Union

import numpy as np

from . import playlist
from .song import Analysis, AnalysisIndex, FeaturesVersion, ProviderError, Song

_SONG_COLUMNS = ("path", "artist", "title", "album", "album_artist", "track_number", "disc_number", "genre", "duration",
                 "version")

Conn = Union[str, sqlite3.Connection]


def _connect(db: Conn) -> Tuple[sqlite3.Connection, bool]:
    if isinstance(db, sqlite3.Connection):
        return db, False
    return sqlite3.connect(db), True


def create_schema(db: Conn) -> None:
    """Tables `song` and `feature` with the columns of src/library.rs:500-531."""
    conn, own = _connect(db)
    try:
        conn.executescript(
            """
            create table if not exists song (
                id integer primary key, path text not null unique, duration float, album_artist text, artist text,
                title text, album text, track_number integer, disc_number integer, genre text, cue_path text,
                audio_file_path text, stamp timestamp default current_timestamp, version integer not null,
                analyzed boolean default false, extra_info json, error text);
            pragma foreign_keys = on;
            create table if not exists feature (
                id integer primary key, song_id integer not null, feature real not null, feature_index integer not null,
                unique(song_id, feature_index), foreign key(song_id) references song(id) on delete cascade);
            """)
        conn.execute("pragma user_version = 5")  # = len(SQLITE_MIGRATIONS): a new database needs no migration
        conn.commit()
    finally:
        if own:
            conn.close()


# SQLITE_MIGRATIONS of the crate (src/library.rs:532-606), by schema version; the statements are the schema contract an
# existing library file obeys, so they are restated as they are.
_MIGRATIONS = (
    "",
    """
    alter table song add column track_number_1 integer;
    update song set track_number_1 = s1.cast_track_number from (
        select cast(track_number as int) as cast_track_number, id from song
    ) as s1 where s1.id = song.id and cast(track_number as int) != 0;
    alter table song drop column track_number;
    alter table song rename column track_number_1 to track_number;
    """,
    "alter table song add column disc_number integer;",
    """
    create table training_triplet (
        id integer primary key, song_1_id integer not null, song_2_id integer not null,
        odd_one_out_id integer not null, stamp timestamp default current_timestamp,
        foreign key(song_1_id) references song(id) on delete cascade,
        foreign key(song_2_id) references song(id) on delete cascade,
        foreign key(odd_one_out_id) references song(id) on delete cascade)
    """,
    """
    create table song_bak (
        id integer primary key, path text not null unique, duration float, album_artist text, artist text,
        title text, album text, track_number integer, disc_number integer, genre text, cue_path text,
        audio_file_path text, stamp timestamp default current_timestamp, version integer not null,
        analyzed boolean default false, extra_info json, error text);
    insert into song_bak (id, path, duration, album_artist, artist, title, album, track_number, disc_number, genre,
                          cue_path, audio_file_path, stamp, version, analyzed, extra_info, error)
        select id, path, duration, album_artist, artist, title, album, track_number, disc_number, genre, cue_path,
               audio_file_path, stamp, coalesce(version, 1), analyzed, extra_info, error from song;
    drop table song;
    alter table song_bak rename to song;
    """,
)


def upgrade(db: Conn) -> int:
    """`Library::upgrade` (src/library.rs:631-681): run the migrations an older database is missing; returns the schema
    version it ends at (5).  A database newer than this mirror is a ProviderError, an empty one gets the current schema."""
    conn, own = _connect(db)
    try:
        version = conn.execute("pragma user_version").fetchone()[0]
        if version > len(_MIGRATIONS):
            raise ProviderError(f"bliss-rs version {version} is older than the schema version {len(_MIGRATIONS)}")
        if version == len(_MIGRATIONS):
            return version
        tables = conn.execute("select count(*) from sqlite_master where type = 'table'").fetchone()[0]
        if version == 0 and tables == 0:
            create_schema(conn)
        else:
            for migration in _MIGRATIONS[version:]:
                conn.executescript(migration)
        conn.execute(f"pragma user_version = {len(_MIGRATIONS)}")
        conn.commit()
        return len(_MIGRATIONS)
    finally:
        if own:
            conn.close()


def load_feature_matrix(db: Conn, features_version: FeaturesVersion = FeaturesVersion.LATEST):
    """-> (song_ids int64[n], paths list[str], matrix float32[n, d]) for the analysed songs of that features version."""
    version = FeaturesVersion(features_version)
    d = version.feature_count()
    conn, own = _connect(db)
    try:
        songs = conn.execute("select id, path from song where analyzed = true and version = ? order by id",
                             (int(version),)).fetchall()
        rows = conn.execute(
            "select feature, song.id from feature join song on song.id = feature.song_id "
            "where song.analyzed = true and song.version = ? order by song_id, feature_index", (int(version),)).fetchall()
    finally:
        if own:
            conn.close()
    ids = np.array([s[0] for s in songs], np.int64)
    feats = np.array([r[0] for r in rows], np.float64)
    owner = np.array([r[1] for r in rows], np.int64)
    # _songs_from_statement (src/library.rs:1297-1345) groups the feature rows by song id and Analysis::new rejects a
    # song that does not carry exactly feature_count() of them, naming the first offender
    counts = {int(i): 0 for i in ids}
    for o in owner:
        counts[int(o)] = counts.get(int(o), 0) + 1
    for (song_id, path) in songs:
        if counts.get(int(song_id), 0) != d:
            raise ProviderError(f"Song with ID {song_id} and path {path} has a different feature number than expected. "
                                "Please rescan or update the song library.")
    return ids, [s[1] for s in songs], feats.astype(np.float32).reshape(ids.size, d)


def load_songs(db: Conn, features_version: FeaturesVersion = FeaturesVersion.LATEST) -> List[Song]:
    """`songs_from_library` (src/library.rs:1355-1372) without the extra_info payload."""
    return _load_songs_and_matrix(db, features_version)[0]


def _load_songs_and_matrix(db: Conn, features_version: FeaturesVersion):
    version = FeaturesVersion(features_version)
    conn, own = _connect(db)
    try:
        ids, _, matrix = load_feature_matrix(conn, version)
        meta = conn.execute(
            f"select {', '.join(_SONG_COLUMNS)}, id from song where analyzed = true and version = ? order by id",
            (int(version),)).fetchall()
    finally:
        if own:
            conn.close()
    out = []
    for row, feats in zip(meta, matrix):
        kw = dict(zip(_SONG_COLUMNS, row[:-1]))
        kw.pop("version")
        kw["duration"] = float(kw["duration"] or 0.0)
        out.append(Song(analysis=Analysis(feats, version), features_version=version, **kw))
    return out, matrix


def store_song(db: Conn, song: Song) -> None:
    """`Library::store_song` (src/library.rs:1560-1630): upsert the song (analyzed = true), replace its features."""
    conn, own = _connect(db)
    try:
        version = FeaturesVersion(song.features_version)
        conn.execute(
            "insert into song (path, artist, title, album, album_artist, track_number, disc_number, genre, duration, "
            "analyzed, version) values (?, ?, ?, ?, ?, ?, ?, ?, ?, true, ?) "
            "on conflict(path) do update set artist=excluded.artist, title=excluded.title, album=excluded.album, "
            "album_artist=excluded.album_artist, track_number=excluded.track_number, disc_number=excluded.disc_number, "
            "genre=excluded.genre, duration=excluded.duration, analyzed=excluded.analyzed, version=excluded.version",
            (song.path, song.artist, song.title, song.album, song.album_artist, song.track_number, song.disc_number,
             song.genre, float(song.duration), int(version)))
        conn.execute("delete from feature where song_id in (select id from song where path = ?)", (song.path,))
        conn.executemany(
            "insert into feature (song_id, feature, feature_index) values ((select id from song where path = ?), ?, ?) "
            "on conflict(song_id, feature_index) do update set feature=excluded.feature",
            [(song.path, float(np.float32(v)), i) for i, v in enumerate(song.analysis.as_vec())])
        conn.commit()
    finally:
        if own:
            conn.close()


def store_songs(db: Conn, songs: Sequence[Song]) -> None:
    conn, own = _connect(db)
    try:
        for s in songs:
            store_song(conn, s)
    finally:
        if own:
            conn.close()


# ---------------------------------------------------------------------------------------------------
# library playlists (src/library.rs:762-893)
# ---------------------------------------------------------------------------------------------------
def _song_from_row(row, feats, version) -> Song:
    kw = dict(zip(_SONG_COLUMNS, row))
    kw.pop("version")
    kw["duration"] = float(kw["duration"] or 0.0)
    return Song(analysis=Analysis(feats, version), features_version=version, **kw)


def songs_from_library(db: Conn, features_version: FeaturesVersion = FeaturesVersion.LATEST) -> List[Song]:
    """`Library::songs_from_library` (src/library.rs:1355-1372): the analysed songs of that features version, by id."""
    return load_songs(db, features_version)


def song_from_path(db: Conn, path: str) -> Song:
    """`Library::song_from_path` (src/library.rs:1414-1460): the analysed song at `path`, whatever its features version."""
    conn, own = _connect(db)
    try:
        row = conn.execute(f"select {', '.join(_SONG_COLUMNS)} from song where path = ? and analyzed = true",
                           (path,)).fetchone()
        if row is None:
            raise ProviderError("Query returned no rows")
        feats = [r[0] for r in conn.execute("select feature from feature join song on song.id = feature.song_id "
                                            "where song.path = ? order by feature_index", (path,))]
    finally:
        if own:
            conn.close()
    version = FeaturesVersion(row[_SONG_COLUMNS.index("version")])
    if len(feats) != version.feature_count():
        raise ProviderError(f"song has more or less than {FeaturesVersion.LATEST.feature_count()} features")
    return _song_from_row(row, np.array(feats, np.float64).astype(np.float32), version)


def songs_from_album(db: Conn, album_title: str, features_version: FeaturesVersion = FeaturesVersion.LATEST) -> List[Song]:
    """`Library::songs_from_album` (src/library.rs:1379-1411): the album's analysed songs of that features version,
    ordered by disc then track number (SQLite: NULL first)."""
    version = FeaturesVersion(features_version)
    conn, own = _connect(db)
    try:
        rows = conn.execute(f"select {', '.join(_SONG_COLUMNS)}, id from song where album = ? and analyzed = true and "
                            "version = ? order by disc_number, track_number", (album_title, int(version))).fetchall()
        feats = {}
        for value, song_id in conn.execute(
                "select feature, song.id from feature join song on song.id = feature.song_id where album = ? and "
                "analyzed = true and version = ? order by song_id, feature_index", (album_title, int(version))):
            feats.setdefault(song_id, []).append(value)
    finally:
        if own:
            conn.close()
    if not rows:
        raise ProviderError("target album was not found in the database.")
    out = []
    for row in rows:
        f = feats.get(row[-1], [])
        if len(f) != version.feature_count():
            raise ProviderError(f"Song with ID {row[-1]} and path {row[0]} has a different feature number than expected. "
                                "Please rescan or update the song library.")
        out.append(_song_from_row(row[:-1], np.array(f, np.float64).astype(np.float32), version))
    return out


def playlist_from(db: Conn, song_paths: Sequence[str]) -> List[Song]:
    """`Library::playlist_from` (src/library.rs:762-767): euclidean distance, closest_to_songs, deduplicated."""
    return playlist_from_custom(db, song_paths, playlist.euclidean_distance, playlist.closest_to_songs, True)


def playlist_from_custom(db: Conn, initial_song_paths: Sequence[str], metric_builder=playlist.euclidean_distance,
                         sort_by=playlist.closest_to_songs, deduplicate: bool = True) -> List[Song]:
    """`Library::playlist_from_custom` (src/library.rs:803-850): the initial songs, then the rest of the library ordered
    by `sort_by(initial_songs, songs, metric_builder)`, deduplicated over the whole chain when `deduplicate`.

    With this package's closest_to_songs / song_to_song the library matrix is read once, the order comes from the device
    and the deduplication is ONE device call over the rows (seeds first) -- no per-song call, no second copy of the rows.
    Any other `sort_by` runs on the host and its result goes through the same single call.  The metric is one of the
    device metrics (playlist._metric_of) or a playlist.ForestOptions.

    A VarianceWeights works with closest_to_songs and deduplicate=False: M = variance_based_weight_matrix(the initial
    songs' analyses) (src/playlist.rs:173-221), at least two initial songs unless few_seeds="euclidean".  deduplicate=True and
    song_to_song are refused: they build one-song metrics.

    A ForestOptions works with closest_to_songs and deduplicate=False (at least two initial songs; the matrix is still read
    once and the forest scores come from the device).  With deduplicate=True the reference would build one-song forests,
    which do not work (src/playlist.rs:230-240, 367-402): ValueError.  To deduplicate a forest playlist, pass the result to
    playlist.dedup_playlist (euclidean).  song_to_song with a forest is refused for the same reason (:285-295)."""
    forest = isinstance(metric_builder, playlist.ForestOptions)
    variance = isinstance(metric_builder, playlist.VarianceWeights)
    if variance:
        if deduplicate:
            playlist._no_variance(metric_builder, "deduplicate=True builds one-song metrics (:367-402); use "
                                                  "playlist.dedup_playlist(result) on the playlist instead")
        if sort_by is playlist.song_to_song:
            playlist._no_variance(metric_builder, "song_to_song rebuilds its metric from one song after the first step (:285-295)")
    if forest:
        if deduplicate:
            playlist._no_forest(metric_builder, "deduplicate=True builds one-song metrics (:367-402); use "
                                                "playlist.dedup_playlist(result) on the playlist instead")
        if sort_by is playlist.song_to_song:
            playlist._no_forest(metric_builder, "song_to_song rebuilds its metric from one song after the first step (:285-295)")
    initial_song_paths = list(initial_song_paths)
    if variance:
        metric_builder.check_counts([len(initial_song_paths)])
    initial = []
    for p in initial_song_paths:
        try:
            initial.append(song_from_path(db, p))
        except Exception as e:
            raise ProviderError(f"song '{p}' has not been analyzed") from e
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    metric, m = (metric_builder, None) if forest or variance else playlist._metric_of(metric_builder)
    chosen = set(initial_song_paths)
    pool = [i for i, s in enumerate(songs) if s.path not in chosen]
    if sort_by not in (playlist.closest_to_songs, playlist.song_to_song):
        ordered = list(sort_by(initial, [songs[i] for i in pool], metric_builder))
        chain = initial + ordered
        return playlist.dedup_playlist_custom_distance(chain, None, metric_builder) if deduplicate else chain
    # the rows of the library; a seed's row is its library row, or appended when it is not one of them (another
    # features version)
    in_library = {s.path for s in songs}
    extra = [s for s in initial if s.path not in in_library]
    rows = songs + extra
    if not rows:
        return []
    if extra:
        X = np.vstack([X] + [np.asarray(s.analysis.as_vec(), np.float32)[None, :] for s in extra])
    row_of = {s.path: i for i, s in enumerate(rows)}
    seed_rows = np.asarray([row_of[s.path] for s in initial], np.int64)
    order = np.zeros(0, np.int64)
    if pool:
        pool_idx = np.asarray(pool, np.int64)
        if sort_by is playlist.closest_to_songs:
            o, _ = playlist.closest_to_songs_order(X[seed_rows], X[pool_idx], metric, m)
        else:
            o = playlist.song_to_song_order(X[seed_rows], X[pool_idx], metric, m)
        order = pool_idx[o.astype(np.int64)]
    seq = np.concatenate([seed_rows, order])
    kept = (playlist.dedup_order(X, seq, playlist.meta_keys(rows), metric, m) if deduplicate
            else np.arange(seq.shape[0]))
    return [initial[k] if k < len(initial) else rows[int(seq[k])] for k in kept]


def similar_songs(db: Conn, k: int, metric_builder=playlist.euclidean_distance, song_paths: Sequence[str] = None):
    """The "similar songs" table of a library: {path: [(path, distance), ...]} with the k songs closest to each song --
    `Library::playlist_from(&[path])?.take(k)` (src/library.rs:762-850, examples/library.rs:194-198) without the seed itself
    and without the deduplication, for every analysed song of FeaturesVersion.LATEST (`song_paths` = None) or for those
    paths only; an unknown path is the ProviderError playlist_from_custom raises.  The matrix is read once and ONE device
    call (playlist.nearest_order, each song skipping its own row) answers every song: no distance matrix is built."""
    playlist._no_forest(metric_builder, "similar_songs builds one metric per song")
    playlist._no_variance(metric_builder, "similar_songs builds one metric per song; use group_playlists for seed sets")
    _, paths, X = load_feature_matrix(db, FeaturesVersion.LATEST)
    metric, m = playlist._metric_of(metric_builder)
    if song_paths is None:
        rows, Q = np.arange(len(paths), dtype=np.int64), X
    else:
        row_of = {p: i for i, p in enumerate(paths)}
        for p in song_paths:
            if p not in row_of:
                raise ProviderError(f"song '{p}' has not been analyzed")
        rows = np.asarray([row_of[p] for p in song_paths], np.int64)
        Q = X[rows]
    if rows.size == 0:
        return {}
    idx, dist = playlist.nearest_order(Q, X, k, metric, m, skip=rows)
    return {paths[int(r)]: [(paths[int(j)], float(v)) for j, v in zip(idx[i], dist[i]) if j >= 0]
            for i, r in enumerate(rows)}


_GROUP_COLUMNS = ("album", "artist", "album_artist", "genre")


def group_playlists(db: Conn, k: int, by: str = "album", metric_builder=playlist.euclidean_distance, groups=None):
    """A k-song playlist for every album (artist, album artist, genre) of a library, or for arbitrary seed sets:
    {key: [(path, score), ...]} where entry `key` is
    `playlist_from_custom(db, paths, metric_builder, closest_to_songs, deduplicate=False)[len(paths):][:k]` with the scores
    (src/library.rs:762-842: the songs closest to the SET of initial songs, the initial songs themselves left out).  The
    library is read once and ONE device call (playlist.nearest_to_groups) answers every group.  With
    metric_builder=playlist.VarianceWeights(...) every group is searched under the variance-based weights of its OWN members
    (src/playlist.rs:173-221), computed on the device in that same call; a group of one song (or none) is the reference's
    ProviderError unless few_seeds="euclidean", decided before the device is touched.

    `by`: the column that groups the analysed songs of FeaturesVersion.LATEST; a song whose key is NULL belongs to no group
    but stays a candidate; groups come in order of first appearance by id, their members in id order.  `groups` =
    {name: [paths]} gives the seed sets instead (a saved playlist): order as given, a repeated path is a seed twice, an
    unknown path is the ProviderError playlist_from_custom raises."""
    playlist._no_forest(metric_builder, "group_playlists takes the distance metrics; forest_playlists builds one forest per group")
    if groups is None and by not in _GROUP_COLUMNS:
        raise ValueError(f"by must be one of {_GROUP_COLUMNS}")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    variance = isinstance(metric_builder, playlist.VarianceWeights)
    metric, m = (metric_builder, None) if variance else playlist._metric_of(metric_builder)
    members = {}
    if groups is None:
        for i, s in enumerate(songs):
            key = getattr(s, by)
            if key is not None:
                members.setdefault(key, []).append(i)
    else:
        row_of = {s.path: i for i, s in enumerate(songs)}
        for name, paths in groups.items():
            for p in paths:
                if p not in row_of:
                    raise ProviderError(f"song '{p}' has not been analyzed")
            members[name] = [row_of[p] for p in paths]
    if not members:
        return {}
    keys = list(members)
    offsets = np.zeros(len(keys) + 1, np.int64)
    offsets[1:] = np.cumsum([len(members[key]) for key in keys])
    rows = np.asarray([i for key in keys for i in members[key]], np.int64)
    idx, dist = playlist.nearest_to_groups((X[rows].reshape(rows.shape[0], X.shape[1]), offsets), X, k, metric, m, skip=rows)
    return {key: [(songs[int(j)].path, float(v)) for j, v in zip(idx[g], dist[g]) if j >= 0] for g, key in enumerate(keys)}


def forest_playlists(db: Conn, k: int, options, by: str = "album", groups=None, few_seeds: str = "raise"):
    """group_playlists with the extended isolation forest (playlist.ForestOptions, src/playlist.rs:230-251), the metric the
    reference means for playlists grown from several seed songs: {key: [(path, score), ...]} where entry `key` is
    `playlist_from_custom(db, paths, options, closest_to_songs, deduplicate=False)[len(paths):][:k]` with the forest scores.
    The library is read once and ONE call (playlist.forest_nearest_to_groups) answers every group: a forest per group, built
    on the host while the device scores the previous ones, the seeds of a group skipped.  Grouping (`by`, `groups`), ordering
    and unknown paths as in group_playlists.

    `few_seeds`: a group with min(sample_size, members) < 2 has no forest, and singles are common in a real library.
    "raise" (the default) is a ValueError, decided before the device is touched; "empty" gives such a group an empty list;
    "euclidean" answers those groups by one playlist.nearest_to_groups call under euclidean_distance -- the scores of THOSE
    rows are euclidean distance sums, not forest scores."""
    if groups is None and by not in _GROUP_COLUMNS:
        raise ValueError(f"by must be one of {_GROUP_COLUMNS}")
    if few_seeds not in ("raise", "empty", "euclidean"):
        raise ValueError('few_seeds must be one of "raise", "empty", "euclidean"')
    if not isinstance(options, playlist.ForestOptions):
        raise TypeError("options must be a playlist.ForestOptions")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    members = {}
    if groups is None:
        for i, s in enumerate(songs):
            key = getattr(s, by)
            if key is not None:
                members.setdefault(key, []).append(i)
    else:
        row_of = {s.path: i for i, s in enumerate(songs)}
        for name, paths in groups.items():
            for p in paths:
                if p not in row_of:
                    raise ProviderError(f"song '{p}' has not been analyzed")
            members[name] = [row_of[p] for p in paths]
    if not members:
        return {}
    keys = list(members)
    counts = [len(members[key]) for key in keys]
    few = playlist._forest_few_seeds(few_seeds, counts, options, ("raise", "empty", "euclidean"))
    offsets = np.zeros(len(keys) + 1, np.int64)
    offsets[1:] = np.cumsum(counts)
    rows = np.asarray([i for key in keys for i in members[key]], np.int64)
    S = X[rows].reshape(rows.shape[0], X.shape[1])
    idx, score = playlist.forest_nearest_to_groups((S, offsets), X, k, options, skip=rows, few_seeds="empty")
    if few_seeds == "euclidean" and few.any():
        sel = np.nonzero(few)[0]
        sub_rows = [rows[offsets[g]:offsets[g + 1]] for g in sel]
        sub_off = np.concatenate([[0], np.cumsum([r.shape[0] for r in sub_rows])]).astype(np.int64)
        flat = np.concatenate(sub_rows + [np.zeros(0, np.int64)])
        sub_idx, sub_dist = playlist.nearest_to_groups((X[flat].reshape(flat.shape[0], X.shape[1]), sub_off), X, k, "euclidean",
                                                       None, skip=flat)
        idx[sel], score[sel] = sub_idx, sub_dist
    return {key: [(songs[int(j)].path, float(v)) for j, v in zip(idx[g], score[g]) if j >= 0] for g, key in enumerate(keys)}


def chain_playlists(db: Conn, k: int, by: str = "song", metric_builder=playlist.euclidean_distance, groups=None,
                    song_paths: Sequence[str] = None):
    """A k-song "journey" playlist starting at every song (album, artist, album artist, genre) of a library, or at arbitrary
    seed sets: {key: [(path, distance), ...]} where entry `key` is
    `playlist_from_custom(db, paths, metric_builder, song_to_song, deduplicate=False)[len(paths):][:k]` (src/playlist.rs:272-326,
    src/library.rs:803-850: the song closest to the SET of initial songs, then from each song to the closest one not played
    yet, the initial songs themselves left out) with the distance that chose each song.  The library is read once and ONE
    device call (playlist.chain_order) answers every key: k steps, not one per song of the library.

    by="song": a chain for every analysed song of FeaturesVersion.LATEST, or for `song_paths` only, keyed by path; each song
    skips its own row.  `by` in album / artist / album_artist / genre, or `groups` = {name: [paths]}: as group_playlists.  An
    unknown path is the ProviderError playlist_from_custom raises.  VarianceWeights and ForestOptions are refused:
    song_to_song rebuilds a one-song metric after the first step."""
    why = "song_to_song rebuilds its metric from one song after the first step (:285-295)"
    playlist._no_forest(metric_builder, why)
    playlist._no_variance(metric_builder, why)
    if groups is None and by != "song" and by not in _GROUP_COLUMNS:
        raise ValueError(f"by must be 'song' or one of {_GROUP_COLUMNS}")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    metric, m = playlist._metric_of(metric_builder)
    row_of = {s.path: i for i, s in enumerate(songs)}
    members = {}
    if groups is not None:
        for name, paths in groups.items():
            for p in paths:
                if p not in row_of:
                    raise ProviderError(f"song '{p}' has not been analyzed")
            members[name] = [row_of[p] for p in paths]
    elif by == "song":
        if song_paths is None:
            members = {s.path: [i] for i, s in enumerate(songs)}
        else:
            for p in song_paths:
                if p not in row_of:
                    raise ProviderError(f"song '{p}' has not been analyzed")
                members[p] = [row_of[p]]
    else:
        for i, s in enumerate(songs):
            key = getattr(s, by)
            if key is not None:
                members.setdefault(key, []).append(i)
    if not members:
        return {}
    keys = list(members)
    offsets = np.zeros(len(keys) + 1, np.int64)
    offsets[1:] = np.cumsum([len(members[key]) for key in keys])
    rows = np.asarray([i for key in keys for i in members[key]], np.int64)
    idx, dist = playlist.chain_order((X[rows].reshape(rows.shape[0], X.shape[1]), offsets), X, k, metric, m, skip=rows)
    return {key: [(songs[int(j)].path, float(v)) for j, v in zip(idx[g], dist[g]) if j >= 0] for g, key in enumerate(keys)}


def _rows_of(songs, paths):
    row_of = {s.path: i for i, s in enumerate(songs)}
    for p in paths:
        if p not in row_of:
            raise ProviderError(f"song '{p}' has not been analyzed")
    return np.asarray([row_of[p] for p in paths], np.int64)


def waypoint_playlists(db: Conn, pairs, k: int, metric_builder=playlist.euclidean_distance) -> List[List[Song]]:
    """For every (from path, to path) of `pairs`, the k songs of the library between the two (playlist.waypoint_playlist: song
    t is the song nearest the point (t + 1) / (k + 1) of the way, none twice, the end points left out), every pair in ONE
    device call (playlist.journey_order) over the analysed songs of FeaturesVersion.LATEST.  -> one list of Songs per pair.
    An unknown path is the ProviderError playlist_from_custom raises.  VarianceWeights and ForestOptions are refused."""
    playlist._no_forest(metric_builder, playlist._JOURNEY_WHY)
    playlist._no_variance(metric_builder, playlist._JOURNEY_WHY)
    pairs = [tuple(p) for p in pairs]
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    ends = _rows_of(songs, [p for pair in pairs for p in pair]).reshape(len(pairs), 2)
    if not pairs:
        return []
    metric, m = playlist._metric_of(metric_builder)
    idx, _ = playlist.journey_order(X[ends[:, 0]], X, k, X[ends[:, 1]], metric, m, skip=ends)
    return [[songs[int(j)] for j in row if j >= 0] for row in idx]


def directed_playlists(db: Conn, k: int, feature=AnalysisIndex.Tempo, direction: str = "down", song_paths: Sequence[str] = None,
                       metric_builder=playlist.euclidean_distance):
    """A directed playlist (playlist.directed_playlist) starting at every analysed song of FeaturesVersion.LATEST, or at
    `song_paths` only: {path: [Song, ...]}, up to k songs, each the nearest song not yet played whose `feature` (an
    AnalysisIndex or a column number) is <= ("down") or >= ("up") that of the song before it; the starting song is left out.
    The library is read once and ONE device call (playlist.journey_order) answers every path.  An unknown path is the
    ProviderError playlist_from_custom raises.  VarianceWeights and ForestOptions are refused."""
    playlist._no_forest(metric_builder, playlist._JOURNEY_WHY)
    playlist._no_variance(metric_builder, playlist._JOURNEY_WHY)
    if direction not in ("up", "down"):
        raise ValueError('direction must be "up" or "down"')
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    paths = [s.path for s in songs] if song_paths is None else list(song_paths)
    rows = _rows_of(songs, paths)
    if not paths:
        return {}
    metric, m = playlist._metric_of(metric_builder)
    skip = np.stack([rows, np.full_like(rows, -1)], axis=1)
    idx, _ = playlist.journey_order(X[rows], X, k, None, metric, m, skip, direction, int(feature))
    return {p: [songs[int(j)] for j in row if j >= 0] for p, row in zip(paths, idx)}


def radio_playlists(db: Conn, k: int, rules=playlist.DEFAULT_RADIO_RULES, song_paths: Sequence[str] = None, mode: str = "chain",
                    metric_builder=playlist.euclidean_distance):
    """A radio (playlist.radio_playlist) starting at every analysed song of FeaturesVersion.LATEST, or at `song_paths` only:
    {path: [Song, ...]}, up to k songs, each the nearest song not yet played (mode "chain": nearest the song before it;
    "nearest": nearest the starting song) that breaks none of `rules` (playlist.Rule; by default no artist twice within 5
    tracks, no album twice within 20).  The starting song is left out of the list and counts as the track before the first.
    The library is read once and ONE device call (playlist.radio_order) answers every path.  An unknown path is the
    ProviderError playlist_from_custom raises.  VarianceWeights and ForestOptions are refused."""
    playlist._no_forest(metric_builder, playlist._RADIO_WHY)
    playlist._no_variance(metric_builder, playlist._RADIO_WHY)
    if mode not in playlist._RADIO_MODES:
        raise ValueError('mode must be "chain" or "nearest"')
    rules = list(rules)
    windows, limits = playlist._rule_arrays(rules, k)
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    paths = [s.path for s in songs] if song_paths is None else list(song_paths)
    rows = _rows_of(songs, paths)
    if not paths:
        return {}
    metric, m = playlist._metric_of(metric_builder)
    labels = playlist.rule_labels(songs, rules)
    skip = np.stack([rows, np.full_like(rows, -1)], axis=1)
    A = X if song_paths is None else X[rows]  # (every song: the rows are the candidates, uploaded once)
    idx, _ = playlist.radio_order(A, X, k, labels, windows, limits, labels[:, rows].T, mode, metric, m, skip)
    return {p: [songs[int(j)] for j in row if j >= 0] for p, row in zip(paths, idx)}


def duplicate_songs(db: Conn, distance_threshold: float = None, metric_builder=playlist.euclidean_distance) -> List[List[Song]]:
    """Which songs of the library are the same song: the duplicate rule of `dedup_playlist_custom_distance`
    (src/playlist.rs:381-388: closer than the threshold, default 0.05, or the same `Some` title and artist) over every pair
    of the analysed songs of FeaturesVersion.LATEST, closed transitively.  -> a list of groups (two or more `Song` each, in
    id order; groups by their first song).  The library is read once (load_songs) and ONE device call answers
    (playlist.duplicate_labels); nothing is deduplicated or deleted."""
    playlist._no_forest(metric_builder, "duplicate_songs builds its metric from single songs")
    playlist._no_variance(metric_builder, "duplicate_songs builds its metric from single songs")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    if not songs:
        return []
    metric, m = playlist._metric_of(metric_builder)
    labels = playlist.duplicate_labels(X, playlist.meta_keys(songs), metric, m, distance_threshold)
    return [[songs[i] for i in g] for g in playlist.groups_from_labels(labels)]


# ---- acoustic fingerprints: a sidecar table beside the crate's (it ignores tables it does not know) ----
def _fingerprint_table(conn) -> None:
    conn.execute("create table if not exists gpu_fingerprint (song_id integer primary key, version integer, words blob)")


def store_fingerprints(db: Conn, fingerprints) -> None:
    """Keep the fingerprints of songs of the library: {path: words} (np.uint32 arrays, as bliss_rs_amd.fingerprint_batch returns
    them) into the sidecar table gpu_fingerprint(song_id, version, words), created on demand; the words are stored little-endian
    with song.FINGERPRINT_VERSION beside them.  A path that is not in the library is a ProviderError; a song's earlier
    fingerprint is replaced."""
    from .song import FINGERPRINT_VERSION

    conn, own = _connect(db)
    try:
        _fingerprint_table(conn)
        for path, words in dict(fingerprints).items():
            row = conn.execute("select id from song where path = ?", (path,)).fetchone()
            if row is None:
                raise ProviderError(f"song '{path}' is not in the library")
            blob = np.ascontiguousarray(words, dtype="<u4").reshape(-1).tobytes()
            conn.execute("insert or replace into gpu_fingerprint (song_id, version, words) values (?, ?, ?)",
                         (int(row[0]), FINGERPRINT_VERSION, blob))
        conn.commit()
    finally:
        if own:
            conn.close()


def load_fingerprints(db: Conn) -> dict:
    """{path: words (np.uint32)} of every song with a stored fingerprint of song.FINGERPRINT_VERSION, in id order; a library
    without the sidecar table has none."""
    from .song import FINGERPRINT_VERSION

    conn, own = _connect(db)
    try:
        if conn.execute("select count(*) from sqlite_master where type = 'table' and name = 'gpu_fingerprint'").fetchone()[0] == 0:
            return {}
        rows = conn.execute("select song.path, gpu_fingerprint.words from gpu_fingerprint join song on song.id = gpu_fingerprint.song_id "
                            "where gpu_fingerprint.version = ? order by song.id", (FINGERPRINT_VERSION,)).fetchall()
    finally:
        if own:
            conn.close()
    return {p: np.frombuffer(bytes(b), dtype="<u4").astype(np.uint32) for p, b in rows}


# ---- loudness: a second sidecar table (bliss_rs_amd.loudness_batch measures, this keeps) ----
def store_loudness(db: Conn, loudness, albums=None) -> None:
    """Keep the loudness of songs of the library: {path: Loudness} into the sidecar table gpu_loudness(song_id, version, lufs,
    range_lu, sample_peak, true_peak, album_lufs, album_peak), created on demand, with song.LOUDNESS_VERSION beside the
    figures.  albums: {path: Loudness}, the figures of the ALBUM each song belongs to (loudness_batch(albums=)'s second
    result, looked up per song); a song without an entry keeps NULL there.  A path that is not in the library is a
    ProviderError; a song's earlier row is replaced.  (SQLite stores -inf, the loudness of digital silence, as it is.)"""
    from .song import LOUDNESS_VERSION

    albums = dict(albums or {})
    conn, own = _connect(db)
    try:
        conn.execute("create table if not exists gpu_loudness (song_id integer primary key, version integer, lufs real, range_lu real, "
                     "sample_peak real, true_peak real, album_lufs real, album_peak real)")
        for path, ld in dict(loudness).items():
            row = conn.execute("select id from song where path = ?", (path,)).fetchone()
            if row is None:
                raise ProviderError(f"song '{path}' is not in the library")
            al = albums.get(path)
            conn.execute("insert or replace into gpu_loudness (song_id, version, lufs, range_lu, sample_peak, true_peak, album_lufs, "
                         "album_peak) values (?, ?, ?, ?, ?, ?, ?, ?)",
                         (int(row[0]), LOUDNESS_VERSION, float(ld.lufs), float(ld.range_lu), float(ld.sample_peak), float(ld.true_peak),
                          None if al is None else float(al.lufs), None if al is None else float(al.true_peak)))
        conn.commit()
    finally:
        if own:
            conn.close()


def load_loudness(db: Conn) -> dict:
    """{path: (Loudness, album_lufs, album_peak)} of every song with a stored row of song.LOUDNESS_VERSION, in id order
    (album_lufs and album_peak are None where none was stored); a library without the sidecar table has none.  The table
    keeps lufs, not the gated power: Loudness.power is 10 ** ((lufs + 0.691) / 10) here, not the measured bits."""
    from .song import LOUDNESS_VERSION, Loudness

    conn, own = _connect(db)
    try:
        if conn.execute("select count(*) from sqlite_master where type = 'table' and name = 'gpu_loudness'").fetchone()[0] == 0:
            return {}
        rows = conn.execute("select song.path, g.lufs, g.range_lu, g.sample_peak, g.true_peak, g.album_lufs, g.album_peak from gpu_loudness g "
                            "join song on song.id = g.song_id where g.version = ? order by song.id", (LOUDNESS_VERSION,)).fetchall()
    finally:
        if own:
            conn.close()
    return {p: (Loudness(lufs=lufs, range_lu=lra, sample_peak=sp, true_peak=tp, power=10.0 ** ((lufs + 0.691) / 10.0)), al, ap)
            for p, lufs, lra, sp, tp, al, ap in rows}


def loudness_statistics(db: Conn) -> dict:
    """How loud the library is, from the stored rows (host arithmetic): {"count", "silent", "lufs": {"mean", "min", "max"},
    "range_lu": {"mean", "min", "max"}}.  Songs of digital silence (lufs -inf) are counted in "silent" and left out of the
    means and extrema; a library without rows has count 0 and None figures.  The loudness range is the number that tells a
    compressed modern master (a few LU) from an orchestral recording (15 LU and more)."""
    stored = load_loudness(db)
    rows = [ld for ld, _, _ in stored.values() if ld.lufs != float("-inf")]

    def summary(values):
        return {"mean": sum(values) / len(values), "min": min(values), "max": max(values)} if values else {"mean": None, "min": None, "max": None}

    return {"count": len(stored), "silent": len(stored) - len(rows), "lufs": summary([ld.lufs for ld in rows]),
            "range_lu": summary([ld.range_lu for ld in rows])}


def fingerprint_candidate_pairs(songs, X, has_fp, k: int, metric_builder=playlist.euclidean_distance) -> np.ndarray:
    """The pairs worth aligning, int64 [P, 2] with i < j, ascending, each once: every fingerprinted song with its k nearest songs by
    features (one playlist.nearest_order call) and the pairs with the same `Some` title and artist (playlist.meta_keys); both
    songs of a pair have a fingerprint."""
    has_fp = np.asarray(has_fp, dtype=bool)
    rows = np.flatnonzero(has_fp)
    found = set()
    if rows.size and int(k) >= 1 and len(songs) >= 2:
        metric, m = playlist._metric_of(metric_builder)
        idx, _ = playlist.nearest_order(X[rows], X, min(int(k), len(songs) - 1), metric, m, skip=rows)
        for r, near in zip(rows.tolist(), idx.tolist()):
            found.update((min(r, j), max(r, j)) for j in near if j >= 0 and has_fp[j])
    by_key = {}
    for i, key in enumerate(playlist.meta_keys(songs).tolist()):
        if key and has_fp[i]:
            by_key.setdefault(key, []).append(i)
    for members in by_key.values():
        found.update((a, b) for n, a in enumerate(members) for b in members[n + 1:])
    return np.asarray(sorted(found), dtype=np.int64).reshape(len(found), 2)


def fingerprint_duplicates(db: Conn, k: int = 10, threshold=playlist.FINGERPRINT_THRESHOLD, metric_builder=playlist.euclidean_distance,
                           max_offset: int = playlist.FINGERPRINT_MAX_OFFSET, min_overlap: int = playlist.FINGERPRINT_MIN_OVERLAP) -> List[List[Song]]:
    """Which songs of the library are the same RECORDING -- a remaster, a compilation copy with another lead-in, an MP3 beside its
    FLAC -- by their stored fingerprints (store_fingerprints) and not by their features, which such copies do not share closely
    enough for duplicate_songs.  Candidates are every fingerprinted song with its k nearest songs by features and the pairs with
    the same `Some` title and artist (fingerprint_candidate_pairs); ONE match call aligns them all
    (playlist.fingerprint_duplicates: bit error rate below `threshold`, default the paper's 0.35).  -> groups of two or more `Song`
    shaped like duplicate_songs' (id order, groups by their first song).  Songs without a fingerprint are in no group."""
    playlist._no_forest(metric_builder, "fingerprint_duplicates ranks its candidates by single songs")
    playlist._no_variance(metric_builder, "fingerprint_duplicates ranks its candidates by single songs")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    stored = load_fingerprints(db)
    if not songs or not stored:
        return []
    fps = [stored.get(s.path, np.zeros(0, np.uint32)) for s in songs]
    has_fp = np.asarray([f.size > 0 for f in fps], dtype=bool)
    pairs = fingerprint_candidate_pairs(songs, X, has_fp, k, metric_builder)
    if pairs.shape[0] == 0:
        return []
    labels = playlist.fingerprint_duplicates(fps, pairs, threshold, max_offset, min_overlap)
    return [[songs[i] for i in g] for g in playlist.groups_from_labels(labels)]


def cluster_songs(db: Conn, k: int, seed: int = 0, metric_builder=playlist.euclidean_distance, max_iter: int = 100,
                  init: str = "k-means++", return_clustering: bool = False):
    """Which k groups the library falls into: k-means (playlist.cluster_songs) over the analysed songs of
    FeaturesVersion.LATEST, read once (load_songs), iterated on the device.  -> k lists of `Song`, cluster c's songs ordered by
    (distance to the cluster's centre, id order): the most typical first; a cluster may be empty.  `return_clustering`: ->
    (lists, playlist.Clustering) with the labels, distances, centres, sizes, n_iter, converged and inertia."""
    playlist._kmeans_metric(metric_builder)  # refused before the database is read
    songs, _ = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    if not songs:
        raise ValueError("cluster_songs needs at least one analysed song")
    clustering = playlist.cluster_songs(songs, k, seed, metric_builder, max_iter, init)
    lists = [[songs[int(i)] for i in clustering.members(c)] for c in range(len(clustering.sizes))]
    return (lists, clustering) if return_clustering else lists


def choose_clusters(db: Conn, ks=range(2, 33), seed: int = 0, metric_builder=playlist.euclidean_distance, max_iter: int = 100,
                    init: str = "k-means++", sample: int = None):
    """Into how many groups the library falls best: playlist.choose_k over the analysed songs of FeaturesVersion.LATEST, read
    once (load_songs) and uploaded once -- k-means and the silhouette of its labels for every k of `ks`, the highest silhouette
    score wins (equal scores: the lower k).  -> (playlist.KSelection, best_k lists of `Song`, each ordered as cluster_songs
    orders them).  `sample`: score that many songs only (drawn with `seed`)."""
    playlist._kmeans_metric(metric_builder)  # refused before the database is read
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    if not songs:
        raise ValueError("choose_clusters needs at least one analysed song")
    sel = playlist.choose_k(X, ks, seed, metric_builder, max_iter, init, sample)
    lists = [[songs[int(i)] for i in sel.clustering.members(c)] for c in range(len(sel.clustering.sizes))]
    return sel, lists


_SILHOUETTE_COLUMNS = ("genre", "album", "artist")


def label_silhouette(db: Conn, by: str = "genre", metric_builder=playlist.euclidean_distance):
    """How well a metric separates the library's genres, albums or artists: the silhouette (playlist.silhouette) of the
    labelling that column gives the analysed songs of FeaturesVersion.LATEST.  Songs whose tag is NULL are left out before the
    call.  -> (playlist.Silhouette, tags): label c is tags[c], in order of first appearance (id order).  Run it with
    euclidean_distance and with MahalanobisBuilder(learn_metric(db, source=by)): the before / after check of a learned M.
    Fewer than two different tags is a ValueError."""
    playlist._silhouette_metric(metric_builder)  # refused before the database is read
    if by not in _SILHOUETTE_COLUMNS:
        raise ValueError(f"by must be one of {_SILHOUETTE_COLUMNS}")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    code, keep, labels = {}, [], []
    for i, s in enumerate(songs):
        tag = getattr(s, by)
        if tag is not None:
            keep.append(i)
            labels.append(code.setdefault(tag, len(code)))
    if len(code) < 2:
        raise ValueError(f"label_silhouette needs songs with at least two different {by} tags")
    return playlist.silhouette(X[np.asarray(keep)], np.asarray(labels, np.int64), metric_builder), list(code)


def _has_triplet_table(conn) -> bool:
    return conn.execute("select count(*) from sqlite_master where type = 'table' and name = 'training_triplet'").fetchone()[0] > 0


def training_triplets(db: Conn, features_version: FeaturesVersion = FeaturesVersion.LATEST) -> np.ndarray:
    """The `training_triplet` table (src/library.rs:542-556: song_1 and song_2 are closer together than they are to
    odd_one_out) as int64[T, 3] row indices (a, b, o) into load_feature_matrix(db, features_version), in id order.  A database
    without the table (create_schema makes none; upgrade of an older file does), or a triplet one of whose songs is not analysed
    at that version, contributes nothing."""
    conn, own = _connect(db)
    try:
        if not _has_triplet_table(conn):
            return np.zeros((0, 3), np.int64)
        ids = [r[0] for r in conn.execute("select id from song where analyzed = true and version = ? order by id",
                                          (int(FeaturesVersion(features_version)),))]
        rows = conn.execute("select song_1_id, song_2_id, odd_one_out_id from training_triplet order by id").fetchall()
    finally:
        if own:
            conn.close()
    row_of = {int(i): k for k, i in enumerate(ids)}
    out = [[row_of[int(v)] for v in r] for r in rows if all(int(v) in row_of for v in r)]
    return np.asarray(out, np.int64).reshape(len(out), 3)


def store_training_triplet(db: Conn, path_1: str, path_2: str, odd_one_out_path: str) -> None:
    """One answer of a survey: the songs at path_1 and path_2 are closer together than either is to odd_one_out_path.  The
    table is created (the crate's migration 4, as it is) when the database has none; an unknown path is a ProviderError."""
    conn, own = _connect(db)
    try:
        ids = []
        for p in (path_1, path_2, odd_one_out_path):
            row = conn.execute("select id from song where path = ?", (p,)).fetchone()
            if row is None:
                raise ProviderError(f"song '{p}' is not in the library")
            ids.append(int(row[0]))
        if not _has_triplet_table(conn):
            conn.execute(_MIGRATIONS[3])
        conn.execute("insert into training_triplet (song_1_id, song_2_id, odd_one_out_id) values (?, ?, ?)", ids)
        conn.commit()
    finally:
        if own:
            conn.close()


_LABEL_COLUMNS = ("genre", "album", "artist", "album_artist")


def learn_metric(db: Conn, source="triplets", form: str = "full", n_triplets: int = None, seed: int = 0, init=None,
                 margin: float = playlist.LEARN_MARGIN, lr: float = playlist.LEARN_LR, reg: float = 0.0,
                 max_iter: int = playlist.LEARN_MAX_ITER, return_result: bool = False):
    """A Mahalanobis matrix for the library, learned on the device (playlist.learn_metric) -> M float32[d, d], ready for
    playlist.MahalanobisBuilder; `return_result`: -> the whole playlist.LearnedMetric.
    source: "triplets" -- the training_triplet table (training_triplets); "genre" / "album" / "artist" / "album_artist" --
    triplets drawn from that column (two songs that share it, one that does not; a song whose value is NULL takes no part);
    a label per analysed song in load_feature_matrix order (an integer array, < 0: no label); or a playlist.Clustering.
    `n_triplets` labelled triplets are drawn with `seed` (playlist.triplets_from_labels; default 10 per song, at least 1000).
    The songs are those of FeaturesVersion.LATEST.  No usable triplet is a ValueError."""
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    if isinstance(source, str) and source == "triplets":
        triplets = training_triplets(db)
    else:
        if isinstance(source, str):
            if source not in _LABEL_COLUMNS:
                raise ValueError(f"source must be 'triplets', one of {_LABEL_COLUMNS}, a label array or a Clustering")
            code = {}
            labels = np.asarray([-1 if getattr(s, source) is None else code.setdefault(getattr(s, source), len(code)) for s in songs],
                                np.int64)
        else:
            labels = np.asarray(source.labels if isinstance(source, playlist.Clustering) else source, np.int64).reshape(-1)
            if labels.shape[0] != len(songs):
                raise ValueError("a label per analysed song is needed")
        triplets = playlist.triplets_from_labels(labels, max(1000, 10 * len(songs)) if n_triplets is None else n_triplets, seed)
    if triplets.shape[0] == 0:
        raise ValueError("learn_metric found no training triplet")
    res = playlist.learn_metric(X, triplets, form, init, margin, lr, reg, max_iter)
    return res if return_result else res.m


def _labels_of(songs, source):
    """a label per song (< 0: none) from a tag column, a label array or a Clustering"""
    if isinstance(source, str):
        if source not in _LABEL_COLUMNS:
            raise ValueError(f"source must be one of {_LABEL_COLUMNS}, a label array or a Clustering")
        code = {}
        return np.asarray([-1 if getattr(s, source) is None else code.setdefault(getattr(s, source), len(code)) for s in songs], np.int64)
    labels = np.asarray(source.labels if isinstance(source, playlist.Clustering) else source, np.int64).reshape(-1)
    if labels.shape[0] != len(songs):
        raise ValueError("a label per analysed song is needed")
    return labels


def covariance_metric(db: Conn, source=None, form: str = "full", shrink: float = playlist.COV_SHRINK, return_result: bool = False):
    """A Mahalanobis matrix for the library in closed form (playlist.covariance_metric) -> M float32[d, d], ready for
    playlist.MahalanobisBuilder; `return_result`: -> the whole playlist.CovarianceMetric.
    source: None -- the inverse of the library's total covariance ("diagonal": every feature standardised, "full": whitened);
    "genre" / "album" / "artist" / "album_artist", a label per analysed song in load_feature_matrix order (< 0: no label) or a
    playlist.Clustering -- the inverse of the pooled covariance WITHIN those groups (songs without a label are left out).
    The songs are those of FeaturesVersion.LATEST.  It needs no iterations and is the baseline to compare learn_metric with."""
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    res = playlist.covariance_metric(X, None if source is None else _labels_of(songs, source), form, shrink)
    return res if return_result else res.m


def statistics(db: Conn, by: str = None):
    """The library's statistics per feature, computed on the device (playlist.moments), in the stored, normalised units.
    by None -> {AnalysisIndex name: {"mean", "std", "min", "max", "count"}} over the analysed songs of FeaturesVersion.LATEST
    (std is the population standard deviation).  by "genre" / "album" / "artist" / "album_artist" -> {tag: that dictionary} for
    every tag of the column; songs whose tag is NULL are left out."""
    if by is not None and by not in _LABEL_COLUMNS:
        raise ValueError(f"by must be None or one of {_LABEL_COLUMNS}")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    names = [AnalysisIndex(r).name for r in range(X.shape[1])]

    def table(mo, g):
        return {name: {"mean": float(mo.mean[g, r]), "std": float(mo.std[g, r]), "min": float(mo.min[g, r]), "max": float(mo.max[g, r]),
                       "count": int(mo.counts[g])} for r, name in enumerate(names)}

    if by is None:
        return table(playlist.moments(X, None, None, False), 0) if len(songs) else {}
    code, keep, labels = {}, [], []
    for i, s in enumerate(songs):
        tag = getattr(s, by)
        if tag is not None:
            keep.append(i)
            labels.append(code.setdefault(tag, len(code)))
    if not code:
        return {}
    mo = playlist.moments(X[np.asarray(keep)], np.asarray(labels, np.int64), len(code), False)
    return {tag: table(mo, g) for tag, g in code.items()}


def album_playlist_from(db: Conn, album_title: str, number_albums: int) -> List[Song]:
    """`Library::album_playlist_from` (src/library.rs:857-893): the album, then the albums closest to it
    (closest_album_to_group), cut after `number_albums` changes of album."""
    album = songs_from_album(db, album_title)
    pl = playlist.closest_album_to_group(album, songs_from_library(db))
    count, index, current = 0, 0, album_title
    for s in pl:
        if s.album != current:
            count += 1
            if count > number_albums:
                break
            current = s.album
        index += 1
    return pl[:index]



def album_playlists(db: Conn, number_albums: int, by: str = "album", groups=None):
    """An album playlist for every album of a library, or for arbitrary seed sets: {key: [Song, ...]} where, with by="album",
    entry `title` has the songs of `album_playlist_from(db, title, number_albums)` in the same order
    (src/library.rs:850-893: the album ordered by disc then track number, then the `number_albums` albums whose mean analysis
    is closest to the album's, each ordered by disc and track number, None first), for every album title of the analysed songs
    of FeaturesVersion.LATEST.  The library is read once and ONE device call (playlist.nearest_albums) answers every key: the
    album means, the group means and the ranking are computed on the device; the reference hard-codes the euclidean distance.

    `by` in artist / album_artist / genre, or `groups` = {name: [paths]}, builds the seed sets as group_playlists does (members
    in id order, or as given); the ranked things are always albums, from which each key's own songs are taken out before the
    means are formed.  An unknown path is the ProviderError playlist_from_custom raises.  number_albums == 0 returns the seed
    songs without touching the device."""
    if groups is None and by not in _GROUP_COLUMNS:
        raise ValueError(f"by must be one of {_GROUP_COLUMNS}")
    number_albums = int(number_albums)
    if number_albums < 0:
        raise ValueError("number_albums must not be negative")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)

    def disc_track(i):  # Option / SQLite: None first
        d, t = songs[i].disc_number, songs[i].track_number
        return ((0, 0) if d is None else (1, d), (0, 0) if t is None else (1, t))

    members = {}
    if groups is None:
        for i, s in enumerate(songs):
            key = getattr(s, by)
            if key is not None:
                members.setdefault(key, []).append(i)
        if by == "album":  # songs_from_album: order by disc_number, track_number
            members = {key: sorted(rows, key=disc_track) for key, rows in members.items()}
    else:
        row_of = {s.path: i for i, s in enumerate(songs)}
        for name, paths in groups.items():
            for p in paths:
                if p not in row_of:
                    raise ProviderError(f"song '{p}' has not been analyzed")
            members[name] = [row_of[p] for p in paths]
    if not members:
        return {}
    keys = list(members)
    if any(not members[key] for key in keys):
        raise ProviderError("Mean of empty slice")
    titles, album_of = {}, np.full(len(songs), -1, np.int64)
    for i, s in enumerate(songs):
        if s.album is not None:
            album_of[i] = titles.setdefault(s.album, len(titles))
    k = min(number_albums, len(titles))
    if k == 0:
        return {key: [songs[i] for i in members[key]] for key in keys}
    if k > 1024:
        raise ValueError("at most 1024 albums per playlist")
    offsets = np.zeros(len(keys) + 1, np.int64)
    offsets[1:] = np.cumsum([len(members[key]) for key in keys])
    rows = np.asarray([i for key in keys for i in members[key]], np.int64)
    idx, _ = playlist.nearest_albums((X[rows].reshape(rows.shape[0], X.shape[1]), offsets), X, album_of, k, skip=rows)
    album_rows = [[] for _ in titles]
    for i, a in enumerate(album_of):
        if a >= 0:
            album_rows[a].append(i)
    out = {}
    for g, key in enumerate(keys):
        gone = set(members[key])
        pl = [songs[i] for i in members[key]]
        for a in idx[g]:
            if a >= 0:
                pl.extend(songs[i] for i in sorted((i for i in album_rows[a] if i not in gone), key=disc_track))
        out[key] = pl
    return out


def _album_disc_track(s):  # Option / SQLite: None first
    a, d, t = s.album, s.disc_number, s.track_number
    return ((0, "") if a is None else (1, a), (0, 0) if d is None else (1, d), (0, 0) if t is None else (1, t))


def _similar_groups(db: Conn, number: int, by: str, metric_builder, mode: str, needed=None):
    """-> (songs, members {key: [row]}, keys, GroupNeighbours or None) for the column `by` of the analysed songs; a `needed` key
    that no song has is a ProviderError, raised before the device is touched"""
    playlist._group_neighbours_metric(metric_builder)  # refused before the database is read
    if by not in _LABEL_COLUMNS:
        raise ValueError(f"by must be one of {_LABEL_COLUMNS}")
    number = int(number)
    if number < 0:
        raise ValueError("number must not be negative")
    if number > 1024:
        raise ValueError("at most 1024 neighbours per group")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    code, members, labels = {}, {}, np.full(len(songs), -1, np.int64)
    for i, s in enumerate(songs):
        tag = getattr(s, by)
        if tag is not None:
            labels[i] = code.setdefault(tag, len(code))
            members.setdefault(tag, []).append(i)
    keys = list(code)
    if needed is not None and needed not in members:
        raise ProviderError(f"target {by} was not found in the database.")
    if number == 0 or len(keys) < 2:
        return songs, members, keys, None
    return songs, members, keys, playlist.group_neighbours(X, labels, min(number, len(keys) - 1), metric_builder, len(keys), None, mode)


def similar_groups(db: Conn, number: int, by: str = "artist", metric_builder=playlist.euclidean_distance, mode: str = "symmetric"):
    """Which artists (albums, genres, album artists) of the library are like each other: {key: [(other_key, distance), ...]} with
    the `number` nearest other keys of every key of the column `by`, nearest first, under the average nearest-member distance
    of playlist.group_neighbours (the reference's TODO.md: "similar artists to the current one").  A set-to-set distance: an
    artist with two styles is near the artists who cover both, where the distance of mean vectors (album_playlists) would put
    it next to artists who sound like neither.  The songs are those of FeaturesVersion.LATEST; songs whose tag is NULL are left
    out.  The library is read once and ONE device call answers every key.  mode "directed": how well the other key covers this
    one.  metric_builder: euclidean_distance or a MahalanobisBuilder."""
    _, _, keys, res = _similar_groups(db, number, by, metric_builder, mode)
    if res is None:
        return {key: [] for key in keys}
    return {key: [(keys[int(c)], float(v)) for c, v in zip(res.idx[g], res.dist[g]) if c >= 0] for g, key in enumerate(keys)}


def similar_artists(db: Conn, number: int, metric_builder=playlist.euclidean_distance, mode: str = "symmetric"):
    """similar_groups with by="artist": {artist: [(other artist, distance), ...]}, nearest first."""
    return similar_groups(db, number, "artist", metric_builder, mode)


def similar_artists_playlist(db: Conn, artist: str, number_artists: int, metric_builder=playlist.euclidean_distance) -> List[Song]:
    """The "similar artists to the current one" playlist of the reference's TODO.md: the artist's songs, then the songs of the
    `number_artists` closest artists (similar_groups, symmetric) in that order, each artist's songs by album, disc and track
    number, None first.  An unknown artist is a ProviderError; number_artists == 0 returns the artist's songs without touching
    the device."""
    number_artists = int(number_artists)
    songs, members, keys, res = _similar_groups(db, number_artists, "artist", metric_builder, "symmetric", artist)
    order = [artist]
    if res is not None:
        order.extend(keys[int(c)] for c in res.idx[keys.index(artist)] if c >= 0)
    return [s for key in order for s in sorted((songs[i] for i in members[key]), key=_album_disc_track)]


def _tree_songs(db: Conn, where):
    """-> (songs, X) of the analysed songs, or of those whose column where[0] has the value where[1]"""
    if where is not None:
        column, value = where
        if column not in _LABEL_COLUMNS:
            raise ValueError(f"where must name one of {_LABEL_COLUMNS}")
    songs, X = _load_songs_and_matrix(db, FeaturesVersion.LATEST)
    if where is not None and songs:
        keep = np.asarray([i for i, s in enumerate(songs) if getattr(s, column) == value], np.int64)
        songs, X = [songs[int(i)] for i in keep], np.ascontiguousarray(X[keep])
    return songs, X


def _song_tree(db: Conn, metric_builder, min_samples, where):
    """-> (songs, playlist.SpanningTree over them)"""
    playlist._mst_metric(metric_builder)  # refused before the database is read
    songs, X = _tree_songs(db, where)
    if not songs:
        return songs, playlist.SpanningTree(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), 0, 0)
    return songs, playlist.minimum_spanning_tree(X, metric_builder, min_samples)


def song_tree(db: Conn, metric_builder=playlist.euclidean_distance, min_samples: int = None, where=None):
    """The minimum spanning tree of the library (playlist.minimum_spanning_tree) over the analysed songs of
    FeaturesVersion.LATEST, read once, in ONE call of the tree (the core distances of min_samples come from the k-nearest
    search first).  -> (paths, playlist.SpanningTree): edge e joins the songs at paths[tree.u[e]] and paths[tree.v[e]], in id
    order.  where = (column, value), such as ("genre", "Jazz"): only the songs whose column has that value."""
    songs, tree = _song_tree(db, metric_builder, min_samples, where)
    return [s.path for s in songs], tree


def linked_clusters(db: Conn, k: int = None, height: float = None, min_cluster_size: int = 1,
                    metric_builder=playlist.euclidean_distance, min_samples: int = None, where=None):
    """Which songs belong together, without a number of clusters and whatever the clusters' shape: the single-linkage clusters
    of the library's spanning tree (song_tree, SpanningTree.cut) at `height`, or the k of them the last k - 1 edges separate.
    -> (lists, unclustered): a list of `Song` per cluster, clusters in order of their first song and songs in id order (the
    shape cluster_songs returns), and the songs of the clusters smaller than min_cluster_size."""
    songs, tree = _song_tree(db, metric_builder, min_samples, where)
    if not songs:
        return [], []
    labels = tree.cut(k, height, min_cluster_size)
    lists, loose = [[] for _ in range(int(labels.max()) + 1)], []
    for s, c in zip(songs, labels):
        (lists[int(c)] if c >= 0 else loose).append(s)
    return lists, loose


def tour(db: Conn, start_path: str = None, where=None, metric_builder=playlist.euclidean_distance, min_samples: int = None) -> List[Song]:
    """Play the whole library (or, with where = ("genre", "Jazz"), one genre) so that each song sounds like one before it: the
    songs in the order of SpanningTree.tour from the song at start_path (None: the first song).  Unlike a greedy
    song-to-song chain the walk never runs out of near songs and jumps.  An unknown start_path -- or one that `where` leaves
    out -- is a ProviderError, raised before the device is touched."""
    playlist._mst_metric(metric_builder)  # refused before the database is read
    songs, X = _tree_songs(db, where)
    start = 0
    if start_path is not None:
        paths = [s.path for s in songs]
        if start_path not in paths:
            raise ProviderError("target song was not found in the database.")
        start = paths.index(start_path)
    if not songs:
        return []
    tree = playlist.minimum_spanning_tree(X, metric_builder, min_samples)
    return [songs[int(i)] for i in tree.tour(start)]


def _ward_tree(db: Conn, metric_builder, where):
    """-> (songs, playlist.WardTree over them)"""
    playlist._ward_metric(metric_builder)  # refused before the database is read
    songs, X = _tree_songs(db, where)
    if not songs:
        return songs, playlist._empty_ward_tree()
    return songs, playlist.ward_tree(X, metric_builder)


def ward_tree(db: Conn, metric_builder=playlist.euclidean_distance, where=None):
    """Ward's dendrogram of the library (playlist.ward_tree) over the analysed songs of FeaturesVersion.LATEST, read once, in ONE
    call of the tree.  -> (paths, playlist.WardTree): merge e joins the clusters whose lowest songs are paths[tree.u[e]] and
    paths[tree.v[e]], in id order.  where = (column, value), such as ("genre", "Jazz"): only the songs whose column has that
    value -- the sub-genres of a genre."""
    songs, tree = _ward_tree(db, metric_builder, where)
    return [s.path for s in songs], tree


def ward_clusters(db: Conn, k: int = None, cost: float = None, min_cluster_size: int = 1, metric_builder=playlist.euclidean_distance,
                  where=None):
    """Which songs belong together, as compact clusters that nest: the clusters of the library's Ward tree (ward_tree,
    WardTree.cut) -- k of them, each a union of clusters of k + 1, or those no merge above `cost` has joined.  -> (lists,
    unclustered): a list of `Song` per cluster, clusters in order of their first song and songs in id order (the shape
    linked_clusters returns), and the songs of the clusters smaller than min_cluster_size."""
    songs, tree = _ward_tree(db, metric_builder, where)
    if not songs:
        return [], []
    labels = tree.cut(k, cost, min_cluster_size)
    lists, loose = [[] for _ in range(int(labels.max()) + 1)], []
    for s, c in zip(songs, labels):
        (lists[int(c)] if c >= 0 else loose).append(s)
    return lists, loose


def medoid_songs(db: Conn, k: int, metric_builder=playlist.euclidean_distance, where=None, return_medoids: bool = False):
    """The k songs that summarise the library: k-medoids (playlist.medoid_songs) over the analysed songs of
    FeaturesVersion.LATEST, read once, every round's all-pairs scan on the device.  Any metric the all-pairs kernel knows:
    playlist.cosine_distance and a MahalanobisBuilder as well as euclidean_distance.  -> (representatives, clusters): k `Song`s
    and, per representative, the songs nearest to it, nearest first.  where = (column, value): only the songs whose column has
    that value.  return_medoids: -> (representatives, clusters, playlist.Medoids)."""
    playlist._pam_metric(metric_builder)  # refused before the database is read
    songs, _ = _tree_songs(db, where)
    if not songs:
        raise ValueError("medoid_songs needs at least one analysed song")
    return playlist.medoid_songs(songs, k, metric_builder, return_medoids=return_medoids)


def _scaled_lists(db: Conn, k, m, kind, metric_builder, scaled=True):
    """-> (paths, idx): every analysed song's k nearest other songs, raw or locally scaled"""
    metric, mm = playlist._scaled_metric(metric_builder, "a per-song search")  # refused before the database is read
    _, paths, X = load_feature_matrix(db, FeaturesVersion.LATEST)
    n = len(paths)
    if n == 0:
        return paths, np.zeros((0, int(k)), np.int64)
    if not scaled:
        return paths, playlist.nearest_order(X, X, k, metric, mm, skip=np.arange(n))[0]
    scale = playlist.local_scales(X, m, kind, metric_builder)
    return paths, playlist.scaled_nearest_order(X, scale, X, scale, k, metric, mm, skip=np.arange(n))[0]


def similar_songs_scaled(db: Conn, k: int, m: int = 10, kind: str = "mean", metric_builder=playlist.euclidean_distance,
                         song_paths: Sequence[str] = None):
    """similar_songs under the locally scaled distance (playlist.scaled_nearest_order): {path: [(path, scaled
    distance), ...]} with the k songs closest to each song when every distance is divided by the geometric mean of the two
    songs' local scales (playlist.local_scales over the m nearest songs of the WHOLE library) -- the lists a few "hub" songs no
    longer dominate.  Two device searches whatever the library: one for the scales, one scaled.  `song_paths`: only those
    songs' lists (the scales still come from the whole library); an unknown path is a ProviderError."""
    metric, mm = playlist._scaled_metric(metric_builder, "similar_songs_scaled")
    _, paths, X = load_feature_matrix(db, FeaturesVersion.LATEST)
    if song_paths is None:
        rows = np.arange(len(paths), dtype=np.int64)
    else:
        row_of = {p: i for i, p in enumerate(paths)}
        for p in song_paths:
            if p not in row_of:
                raise ProviderError(f"song '{p}' has not been analyzed")
        rows = np.asarray([row_of[p] for p in song_paths], np.int64)
    if rows.size == 0:
        return {}
    scale = playlist.local_scales(X, m, kind, metric_builder)
    if song_paths is None:
        idx, dist = playlist.scaled_nearest_order(X, scale, X, scale, k, metric, mm, skip=rows)
    else:
        idx, dist = playlist.scaled_nearest_order(X[rows], scale[rows], X, scale, k, metric, mm, skip=rows)
    return {paths[int(r)]: [(paths[int(j)], float(v)) for j, v in zip(idx[i], dist[i]) if j >= 0]
            for i, r in enumerate(rows)}


def hubness(db: Conn, k: int, scaled: bool = False, m: int = 10, kind: str = "mean", metric_builder=playlist.euclidean_distance):
    """How unevenly the library's similar-songs lists spread their recommendations: -> (playlist.Hubness, paths) over every
    analysed song's k nearest other songs, raw (`scaled` False: what similar_songs returns) or locally scaled (what
    similar_songs_scaled returns).  hubness.counts[i] is the number of lists the song at paths[i] is in, hubness.skewness the
    one number to compare two similarity measures by, hubness.hubs(t) the rows of the songs that dominate."""
    paths, idx = _scaled_lists(db, k, m, kind, metric_builder, scaled)
    if not paths:
        return playlist.Hubness.from_counts(np.zeros(0, np.int64), k), paths
    return playlist.hubness(idx, len(paths)), paths


def orphan_songs(db: Conn, k: int, scaled: bool = False, m: int = 10, kind: str = "mean",
                 metric_builder=playlist.euclidean_distance) -> List[str]:
    """The paths no song's list of k similar songs contains -- the part of a library a recommender never plays --, raw or
    locally scaled, in id order."""
    h, paths = hubness(db, k, scaled, m, kind, metric_builder)
    return [paths[int(i)] for i in h.orphans()]


def song_map(db: Conn, perplexity: float = 30.0, n_iter: int = 750, metric_builder=playlist.euclidean_distance, init="pca", **options):
    """A picture of the library (playlist.song_map) over the analysed songs of FeaturesVersion.LATEST, read
    once: -> (playlist.SongMap, paths); the point of the song at paths[i] is map.xy[i], in id order, for a front end to draw
    and colour by genre, album or cluster.  `options` are song_map's further parameters (exag_iters, learning_rate, ...)."""
    playlist._scaled_metric(metric_builder, "song_map")  # refused before the database is read
    _, paths, X = load_feature_matrix(db, FeaturesVersion.LATEST)
    if not paths:
        return playlist.SongMap(np.zeros((0, 2), np.float32), np.zeros(max(int(n_iter), 0), np.float64), 0.0), paths
    return playlist.song_map(X, perplexity, n_iter, metric_builder, init, **options), paths
