// stage_io.hpp -- the two ways a file-sized array crosses the link outside a run, through page-locked
// staging buffers of RS_IO_STAGE bytes:
//   StageIn           host bytes (a file through pread, the caller's arrays, the engine's log) -> device,
//                     a ring of kStageBufs buffers on the copy stream (pin slot kPinStage)
//   ImageOut          a device image -> a file, a ring of kBufs buffers on the caller's stream that four
//                     threads pwrite (pin slot kPinWrite)
//   write_image_file  the file around such an image: head, image, tail
// and the guards both use (Events, StreamDrain; Fd, pread_all and pwrite_all are host_common.hpp's).
// The --O0 .r1cs reader, the .sym, JSON and .wtns writers, the .r1cs writer and the witness calls are all
// callers; the run's own upload and result stream have their own rings (load_enqueue, snap_*).
#pragma once
// (included by engine.hip inside namespace rs, after pin_get's declaration)

// N events, created here and destroyed with the scope
template <int N>
struct Events {
  hipEvent_t e[N] = {};
  explicit Events(unsigned flags = hipEventDisableTiming) {
    for (hipEvent_t &x : e) {
      const hipError_t rc = hipEventCreateWithFlags(&x, flags);
      if (rc != hipSuccess) {
        clear();
        throw RsError(RS_E_HIP, std::string("hipEventCreateWithFlags: ") + hipGetErrorString(rc));
      }
    }
  }
  ~Events() { clear(); }
  Events(const Events &) = delete;
  Events &operator=(const Events &) = delete;
  void clear() {
    for (hipEvent_t &x : e) {
      if (x) (void)hipEventDestroy(x);
      x = nullptr;
    }
  }
};

// Nothing is left queued on `s` on any way out of the scope (a throw included): what the stream reads
// and writes -- a staging pool, the caller's buffers -- is free again
struct StreamDrain {
  hipStream_t s;
  ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// RS_IO_STAGE: bytes a staging buffer, in and out (read on every call; tests shrink it so that both rings
// wrap on small files).  A power of two (rounded down); the floor keeps a buffer a whole number of the
// largest .sym chunks (sym_write.hpp asserts it).
constexpr uint64_t kIoStage = 32ull << 20, kIoStageMin = 64ull << 10;
constexpr int kStageBufs = 4;
static uint64_t io_stage() {
  uint64_t s = env_u64("RS_IO_STAGE", kIoStage, kIoStageMin, kIoStage);
  while (s & (s - 1)) s &= s - 1;
  return s;
}

// ---------------------------------------------------------------- host bytes on their way to the device
// The ring lives for one call: made from the bytes it will carry in all (the pool is kStageBufs buffers of
// min(RS_IO_STAGE, bytes)), and the copy stream is drained on every way out of its scope.  `unit`: a
// buffer holds a whole number of units (a witness value, a .sym chunk).
struct StageIn {
  rs_engine *E;
  uint64_t stage;    // bytes a buffer
  uint8_t *pool;
  uint64_t seq = 0;  // pieces sent so far, over every send: piece seq uses buffer seq % kStageBufs
  Events<kStageBufs> ev;
  StreamDrain drain;  // (after ev: the stream is drained before the events go)
  StageIn(rs_engine *E_, uint64_t bytes, uint64_t unit = 1)
      : E(E_), stage(std::min(io_stage() / unit * unit, bytes)), pool((uint8_t *)pin_get(E_, kPinStage, kStageBufs * stage)), drain{E_->stc} {}
  // `bytes` bytes to dst_dev in pieces of at most one buffer.  A piece: wait for the buffer's previous
  // copy (once the ring has wrapped); fill(buf, off, len) -> bool puts bytes [off, off + len) into the
  // buffer (false: RS_E_INVALID with `cannot_read`); the H2D and the buffer's event on the copy stream;
  // then(buf, off, len), for what the caller queues behind the piece or wants to see of it.
  template <class Fill, class Then>
  void send(void *dst_dev, uint64_t bytes, const std::string &cannot_read, Fill &&fill, Then &&then) {
    for (uint64_t off = 0; off < bytes; off += stage, ++seq) {
      uint8_t *buf = pool + (seq % kStageBufs) * stage;
      const hipEvent_t copied = ev.e[seq % kStageBufs];
      if (seq >= (uint64_t)kStageBufs) HC(hipEventSynchronize(copied));
      const uint64_t len = std::min(stage, bytes - off);
      if (!fill(buf, off, len)) throw RsError(RS_E_INVALID, cannot_read);
      HC(hipMemcpyAsync((uint8_t *)dst_dev + off, buf, len, hipMemcpyHostToDevice, E->stc));
      HC(hipEventRecord(copied, E->stc));
      then((const uint8_t *)buf, off, len);
    }
  }
  template <class Fill>
  void send(void *dst_dev, uint64_t bytes, const std::string &cannot_read, Fill &&fill) {
    send(dst_dev, bytes, cannot_read, fill, [](const uint8_t *, uint64_t, uint64_t) {});
  }
  // a host array
  void send(void *dst_dev, const void *src, uint64_t bytes) {
    send(dst_dev, bytes, "", [src](uint8_t *buf, uint64_t off, uint64_t len) { memcpy(buf, (const uint8_t *)src + off, len); return true; });
  }
};

// ---------------------------------------------------------------- a device image on its way to a file
// RS_IO_STAGE-byte chunks through page-locked buffers that four threads pwrite at their offsets while the
// next chunks' D2H run.  The page cache bounds it: on the GPU box's overlay file system a fresh 0.92 GB file
// takes 130-160 ms with one or four writers (a shared mapping with four copiers: ~400 ms of page faults),
// the D2H ~18 ms at link speed.
struct ImageOut {
  static constexpr int kBufs = 8, kThreads = 4;
  uint64_t chunk = 0;
  uint8_t *pool = nullptr;
  Events<kBufs> ev;
  // Everything that can throw before the file exists -- the events (made with the object), the pinned
  // buffers here -- so construct and prepare before open() (a throw between open() and the
  // guarded block leaked the fd or destroyed joinable threads)
  void prepare(rs_engine *E, uint64_t bytes) {
    chunk = io_stage();
    const uint64_t nch = (bytes + chunk - 1) / chunk;
    if (nch) pool = (uint8_t *)pin_get(E, kPinWrite, nch > 1 ? std::min<uint64_t>(nch, kBufs) * chunk : bytes);
  }
  // src[0, bytes) (device; its producers on `st`) -> fd at img_off; a failed write sets io_err
  void run(hipStream_t st, int fd, const uint8_t *src, uint64_t bytes, uint64_t img_off, std::atomic<bool> &io_err) {
    const uint64_t nch = (bytes + chunk - 1) / chunk;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<uint64_t> work;       // chunks whose D2H is enqueued
    std::vector<char> written(nch, 0);
    bool closing = false;
    // the writer threads are joined on every way out of this scope (a throw included): closing drains
    // them, and the guard lives after everything they reference
    struct Writers {
      std::vector<std::thread> th;
      std::mutex &mu;
      std::condition_variable &cv;
      bool &closing;
      std::deque<uint64_t> &work;
      void stop(bool drop) {
        {
          std::lock_guard<std::mutex> lk(mu);
          closing = true;
          if (drop) work.clear();
        }
        cv.notify_all();
        for (auto &x : th)
          if (x.joinable()) x.join();
      }
      ~Writers() { stop(true); }
    } writers{{}, mu, cv, closing, work};
    for (int t = 0; t < kThreads && (uint64_t)t < nch; ++t)
      writers.th.emplace_back([&]() {
        for (;;) {
          uint64_t i;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return closing || !work.empty(); });
            if (work.empty()) return;
            i = work.front();
            work.pop_front();
          }
          const uint64_t off = i * chunk, len = std::min(chunk, bytes - off);
          if (hipEventSynchronize(ev.e[i % kBufs]) != hipSuccess) io_err = true;
          else if (!pwrite_all(fd, pool + (i % kBufs) * chunk, len, img_off + off)) io_err = true;
          {
            std::lock_guard<std::mutex> lk(mu);
            written[i] = 1;
          }
          cv.notify_all();
        }
      });
    for (uint64_t i = 0; i < nch; ++i) {
      if (i >= (uint64_t)kBufs) {  // the buffer's previous chunk is on disk
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return written[i - kBufs] != 0; });
      }
      const uint64_t off = i * chunk, len = std::min(chunk, bytes - off);
      HC(hipMemcpyAsync(pool + (i % kBufs) * chunk, src + off, len, hipMemcpyDeviceToHost, st));
      HC(hipEventRecord(ev.e[i % kBufs], st));
      {
        std::lock_guard<std::mutex> lk(mu);
        work.push_back(i);
      }
      cv.notify_all();
    }
    writers.stop(false);  // every chunk written
  }
};

struct Bytes {
  const void *p = nullptr;
  uint64_t n = 0;
};
// The file at `path`: head, the device image img[0, bytes) (its producers on `st`), tail.  The file's
// blocks are asked for up front, while the image's last kernel may still run (a fresh 0.92 GB file: 10.0 ->
// 11.4 GB/s from host memory on the GPU box's /tmp, tools/writer_bench.py); a file system without
// fallocate gets the size by ftruncate.  before_image (optional): called once the file stands, before a
// non-empty image leaves -- where a writer waits for its last kernel and reads its events' times.
static void write_image_file(rs_engine *E, const char *path, Bytes head, Bytes tail, const void *img, uint64_t bytes, hipStream_t st,
                             const std::function<void()> &before_image = nullptr) {
  ImageOut io;
  io.prepare(E, bytes);
  Fd dst;
  dst.fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (dst.fd < 0) throw RsError(RS_E_INVALID, std::string("cannot write ") + path);
  std::atomic<bool> io_err{false};
  const uint64_t fsize = head.n + bytes + tail.n;
  if (fsize && posix_fallocate(dst.fd, 0, (off_t)fsize) != 0 && ftruncate(dst.fd, (off_t)fsize) != 0) io_err = true;
  if (!pwrite_all(dst.fd, head.p, head.n, 0)) io_err = true;
  if (!pwrite_all(dst.fd, tail.p, tail.n, head.n + bytes)) io_err = true;
  if (bytes) {
    if (before_image) before_image();
    io.run(st, dst.fd, (const uint8_t *)img, bytes, head.n, io_err);
  }
  if (close(dst.release()) != 0) io_err = true;
  if (io_err) throw RsError(RS_E_INVALID, "write error");
}
