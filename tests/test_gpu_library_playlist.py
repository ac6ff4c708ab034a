"""GPU tests (-m gpu) of the library playlists (bliss_rs_amd.library.playlist_from / playlist_from_custom /
album_playlist_from / songs_from_album, src/library.rs:762-893, 1379-1411): the reference's own test library
(tests/golden/library_playlist_cases.json, setup_test_library) written to a temporary SQLite file, every expected path
list asserted exactly."""
import json
import os
import sqlite3

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "library_playlist_cases.json")))


@pytest.fixture(scope="module")
def bliss():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import bliss_rs_amd

    return bliss_rs_amd


@pytest.fixture(scope="module")
def db(bliss, tmp_path_factory):
    """Rows in id order, so that `order by id` sees the reference's order: the analysed current-version songs through
    store_song, the others (not analysed, Version1, short feature lists) in plain SQL."""
    path = str(tmp_path_factory.mktemp("library") / "bliss.db")
    L = bliss.library
    L.create_schema(path)
    conn = sqlite3.connect(path)
    for r in sorted(FIXTURE["rows"], key=lambda r: r["id"]):
        if r["analyzed"] and r["version"] == 2 and len(r["features"]) == 23:
            song = bliss.Song(path=r["path"], artist=r["artist"], title=r["title"], album=r["album"],
                              album_artist=r["album_artist"], track_number=r["track_number"], disc_number=r["disc_number"],
                              genre=r["genre"], duration=float(r["duration"]),
                              analysis=bliss.Analysis(r["features"], bliss.FeaturesVersion.Version2),
                              features_version=bliss.FeaturesVersion.Version2)
            L.store_song(conn, song)
            conn.execute("update song set extra_info = ?, cue_path = ?, audio_file_path = ? where path = ?",
                         (r["extra_info"], r["cue_path"], r["audio_file_path"], r["path"]))
        else:
            conn.execute(
                "insert into song (id, path, artist, title, album, album_artist, track_number, disc_number, genre, duration, "
                "analyzed, version, extra_info, cue_path, audio_file_path, error) values (?, ?, ?, ?, ?, ?, ?, ?, ?, ?, ?, ?, ?, "
                "?, ?, ?)", tuple(r[k] for k in ("id", "path", "artist", "title", "album", "album_artist", "track_number",
                                                  "disc_number", "genre", "duration", "analyzed", "version", "extra_info",
                                                  "cue_path", "audio_file_path", "error")))
            conn.executemany("insert into feature (song_id, feature, feature_index) values (?, ?, ?)",
                             [(r["id"], v, i) for i, v in enumerate(r["features"])])
    conn.commit()
    conn.close()
    return path


def _run(bliss, db, case):
    L, P = bliss.library, bliss.playlist
    if case["call"] == "playlist_from":
        return L.playlist_from(db, case["paths"])
    if case["call"] == "playlist_from_custom":
        sort_by = {"closest_to_songs": P.closest_to_songs, "song_to_song": P.song_to_song,
                   "path": lambda _initial, songs, _metric: sorted(songs, key=lambda s: s.path)}[case["sort_by"]]
        return L.playlist_from_custom(db, case["paths"], {"euclidean": P.euclidean_distance}[case["metric"]], sort_by,
                                      case["deduplicate"])
    if case["call"] == "album_playlist_from":
        return L.album_playlist_from(db, case["album"], case["number_albums"])
    return L.songs_from_album(db, case["album"])


@pytest.mark.parametrize("name", sorted(FIXTURE["cases"]))
def test_reference_library_case(bliss, db, name):
    case = FIXTURE["cases"][name]
    if "error" in case:
        with pytest.raises(bliss.ProviderError) as e:
            _run(bliss, db, case)
        assert e.value.message == case["error"]
        return
    got = [s.path for s in _run(bliss, db, case)]
    assert got[:case.get("take", len(got))] == case["expected"]


def test_library_playlist_is_one_dedup_call(bliss, db, monkeypatch):
    """playlist_from: the order on the device, then ONE deduplication call over seeds + ordered candidates."""
    from bliss_rs_amd import _ffi

    L = _ffi.lib()
    calls = {"blissgpu_dedup_playlist": 0, "blissgpu_set_distance": 0, "blissgpu_closest_to_songs": 0}
    for name in calls:
        fn = getattr(L, name)

        def counted(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)

        monkeypatch.setattr(L, name, counted)
    got = [s.path for s in bliss.library.playlist_from(db, ["/path/to/song2001"])]
    assert got == FIXTURE["cases"]["test_library_simple_playlist"]["expected"]
    assert calls == {"blissgpu_dedup_playlist": 1, "blissgpu_set_distance": 0, "blissgpu_closest_to_songs": 1}


def test_song_to_song_and_song_objects(bliss, db):
    """song_to_song as sort_by takes the device path too; the results are the library's songs with their metadata, the
    seeds the songs song_from_path returns."""
    L, P = bliss.library, bliss.playlist
    pl = L.playlist_from_custom(db, ["/path/to/song1001"], P.euclidean_distance, P.song_to_song, True)
    songs = L.songs_from_library(db)
    ref = P.dedup_playlist_custom_distance(
        [L.song_from_path(db, "/path/to/song1001")]
        + P.song_to_song([L.song_from_path(db, "/path/to/song1001")], [s for s in songs if s.path != "/path/to/song1001"]))
    assert [s.path for s in pl] == [s.path for s in ref]
    assert pl[0] == L.song_from_path(db, "/path/to/song1001")
    assert all(s in songs for s in pl[1:])
    with pytest.raises(bliss.ProviderError, match="has not been analyzed"):
        L.playlist_from(db, ["/path/to/song3001"])  # in the database, not analysed
